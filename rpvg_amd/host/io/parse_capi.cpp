// C entry points over the readers of the --write-probs dump (harness: tests and tools bind them with ctypes).  Every reader ends
// in the same flat arrays (FlatDump), so two of them are compared byte for byte:
//   rpvg_amd_rows_parse             the device parse (ParsedDump), flat from its views
//   rpvg_amd_rows_parse_host_line   readProbabilityClusters on one host thread, flattened: the reader the device parse replaces.  No GPU.
//   rpvg_amd_rows_parse_plan        the functions of rpvg_amd/csrc/rows_parse_plan.hpp over serial scans: what the kernels compute,
//                                   without a GPU (and the refusal, as "line <n>: <reason>")
//   rpvg_amd_rows_parse_file        a file through readProbabilityClustersDevice or readProbabilityClusters, flattened

#include <chrono>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../hip_engine.hpp"
#include "../runner_handles.hpp"
#include "../../csrc/rows_parse_plan.hpp"
#include "cluster_io.hpp"

using namespace rpvg_amd;
using namespace rpvg_amd_harness;

namespace {

thread_local std::string parse_last_error;

struct FlatDump {

    std::vector<uint64_t> cluster_row_off, cluster_path_off, row_grp_off, grp_idx_off, name_off, num_align_lists, cluster_index;
    std::vector<uint32_t> row_count, path_idx, path_length;
    std::vector<double> row_noise, grp_prob, path_effective_length;
    std::vector<uint8_t> has_rank_key;
    std::string name_bytes;
    double seconds = 0;
};

FlatDump flatten(const std::vector<ProbabilityCluster> & clusters) {

    FlatDump out;
    out.cluster_row_off.push_back(0);
    out.cluster_path_off.push_back(0);
    out.row_grp_off.push_back(0);
    out.grp_idx_off.push_back(0);
    out.name_off.push_back(0);

    for (auto & cluster: clusters) {

        out.has_rank_key.push_back(cluster.has_rank_key ? 1 : 0);
        out.num_align_lists.push_back(cluster.num_align_lists);
        out.cluster_index.push_back(cluster.cluster_index);

        for (auto & path: cluster.paths) {

            out.name_bytes += path.name;
            out.name_off.push_back(out.name_bytes.size());
            out.path_length.push_back(path.length);
            out.path_effective_length.push_back(path.effective_length);
        }

        for (auto & row: cluster.cluster_probs) {

            out.row_count.push_back(row.readCount());
            out.row_noise.push_back(row.noiseProb());

            for (auto & group: row.pathProbs()) {

                out.grp_prob.push_back(group.first);
                out.path_idx.insert(out.path_idx.end(), group.second.begin(), group.second.end());
                out.grp_idx_off.push_back(out.path_idx.size());
            }

            out.row_grp_off.push_back(out.grp_prob.size());
        }

        out.cluster_path_off.push_back(out.path_length.size());
        out.cluster_row_off.push_back(out.row_count.size());
    }

    return out;
}

FlatDump flatten(const ParsedDump & dump) {

    const rpvg_parsed_dump_view paths = dump.view();
    const rpvg_cluster_batch rows = dump.rowsView();
    const uint64_t K = paths.num_clusters, P = paths.num_paths, R = rows.cluster_row_off[K];
    const uint64_t G = R ? rows.row_grp_off[R] : 0, M = G ? rows.grp_idx_off[G] : 0;

    FlatDump out;
    out.cluster_row_off.assign(rows.cluster_row_off, rows.cluster_row_off + K + 1);
    out.cluster_path_off.assign(paths.cluster_path_off, paths.cluster_path_off + K + 1);
    out.row_grp_off.assign(1, 0);
    out.grp_idx_off.assign(1, 0);
    if (R) out.row_grp_off.assign(rows.row_grp_off, rows.row_grp_off + R + 1);
    if (R) out.grp_idx_off.assign(rows.grp_idx_off, rows.grp_idx_off + G + 1);
    out.name_off.assign(paths.name_off, paths.name_off + P + 1);
    out.num_align_lists.assign(paths.num_align_lists, paths.num_align_lists + K);
    out.cluster_index.assign(paths.cluster_index, paths.cluster_index + K);
    out.has_rank_key.assign(paths.has_rank_key, paths.has_rank_key + K);
    out.path_length.assign(paths.path_length, paths.path_length + P);
    out.path_effective_length.assign(paths.path_effective_length, paths.path_effective_length + P);
    out.name_bytes.assign(paths.name_bytes, paths.num_name_bytes);
    if (R) out.row_count.assign(rows.row_count, rows.row_count + R);
    if (R) out.row_noise.assign(rows.row_noise, rows.row_noise + R);
    if (G) out.grp_prob.assign(rows.grp_prob, rows.grp_prob + G);
    if (M) out.path_idx.assign(rows.path_idx, rows.path_idx + M);
    return out;
}

// the kernels' functions over serial scans
struct HostSink {

    rpvg_hip_detail::word64 bad = rpvg_hip_detail::kNoBad;
    uint64_t name_bytes = 0, exact = 0;

    void report(const uint32_t line_start, const int why) { bad = std::min(bad, rpvg_hip_detail::offenderWord(line_start, why)); }
    void nameBytes(const uint32_t n) { name_bytes += n; }
    void exactToken() { exact += 1; }
};

FlatDump planParse(const char * text, const uint64_t num_bytes, uint64_t * exact_out) {

    namespace pp = rpvg_rows_parse;

    if (num_bytes > pp::kMaxTextBytes) {

        throw std::runtime_error("a text of 2^31 - 1 bytes or more");
    }

    const uint32_t n = num_bytes;
    std::vector<uint32_t> scans[9];

    for (auto & scan: scans) {

        scan.assign(static_cast<size_t>(n) + 1, 0);
    }

    for (uint32_t i = 0; i < n; ++i) {

        pp::rawFlags(text, i, scans[0].data(), scans[1].data(), scans[2].data(), scans[3].data());
    }

    for (int a = 0; a < 4; ++a) {

        for (uint32_t i = 1; i < n; ++i) {

            scans[a][i] = std::max(scans[a][i], scans[a][i - 1]);
        }
    }

    const pp::Scanned x = {text, n, scans[0].data(), scans[1].data(), scans[2].data(), scans[3].data()};

    for (uint32_t i = 0; i < n; ++i) {

        pp::countFlags(x, i, scans[4].data(), scans[5].data(), scans[6].data(), scans[7].data(), scans[8].data());
    }

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

    const pp::Counted c = {scans[4].data(), scans[5].data(), scans[6].data(), scans[7].data(), scans[8].data()};
    const uint64_t K = totals[0], P = totals[1], R = totals[2], G = totals[3], M = totals[4];

    FlatDump out;
    out.cluster_row_off.assign(K + 1, 0);
    out.cluster_path_off.assign(K + 1, 0);
    out.has_rank_key.assign(K, 0);
    out.num_align_lists.assign(K, 0);
    out.cluster_index.assign(K, 0);
    out.name_off.assign(P + 1, 0);
    out.path_length.assign(P, 0);
    out.path_effective_length.assign(P, 0);
    out.row_count.assign(R, 0);
    out.row_noise.assign(R, 0);
    out.row_grp_off.assign(R + 1, 0);
    out.grp_prob.assign(G, 0);
    out.grp_idx_off.assign(G + 1, 0);
    out.path_idx.assign(M, 0);

    std::vector<uint32_t> cluster_id(K), name_src(P), text_idx(M), row_unsorted(R, 0), row_line(R, 0);
    std::vector<double> text_prob(G);
    std::vector<uint64_t> text_idx_off(G + 1, 0), source(G);
    std::vector<uint64_t> pow10(rpvg_number_text::kPow10Words);
    rpvg_number_text::buildPow10Table(pow10.data(), nullptr);

    pp::Parsed o = {};
    o.K = K;
    o.P = P;
    o.R = R;
    o.G = G;
    o.M = M;
    o.cluster_row_off = out.cluster_row_off.data();
    o.cluster_path_off = out.cluster_path_off.data();
    o.has_rank_key = out.has_rank_key.data();
    o.num_align_lists = out.num_align_lists.data();
    o.cluster_index = out.cluster_index.data();
    o.cluster_id = cluster_id.data();
    o.name_len = out.name_off.data();
    o.name_src = name_src.data();
    o.path_length = out.path_length.data();
    o.path_effective_length = out.path_effective_length.data();
    o.row_count = out.row_count.data();
    o.row_noise = out.row_noise.data();
    o.row_grp_off = out.row_grp_off.data();
    o.row_line = row_line.data();
    o.text_prob = text_prob.data();
    o.text_idx_off = text_idx_off.data();
    o.text_idx = text_idx.data();
    o.pow10 = pow10.data();

    for (uint32_t i = 0; i < n; ++i) {

        pp::markerByte(x, c, o, i);
    }

    HostSink sink;

    for (uint32_t i = 0; i < n; ++i) {

        pp::fillByte(x, c, o, i, sink);
    }

    if (exact_out) {

        *exact_out = sink.exact;
    }

    const auto refuseIfBad = [&]() {

        if (sink.bad != rpvg_hip_detail::kNoBad) {

            const auto offender = rpvg_hip_detail::offenderOf(sink.bad, pp::kWhyLast);
            uint64_t line = 1;

            for (uint64_t i = 0; i < offender.index; ++i) {

                line += text[i] == '\n';
            }

            throw std::runtime_error("line " + std::to_string(line) + ": " + pp::reasonOf(offender.why));
        }
    };

    refuseIfBad();

    const pp::Groups q = {R, G, M, out.row_grp_off.data(), text_prob.data(), text_idx_off.data(), text_idx.data(), row_unsorted.data(), source.data(), out.grp_idx_off.data()};
    out.grp_idx_off[G] = M;

    for (uint64_t g = 0; g < G; ++g) {

        pp::orderGroup(q, g, [&](const uint64_t r) { row_unsorted[r] = 1; });
    }

    for (uint64_t r = 0; r < R; ++r) {

        pp::sortRow(q, r, [&](const uint64_t row) { sink.report(row_line[row], pp::kWhyUnsortedRow); });
    }

    refuseIfBad();  // (an unsorted row too long to sort)

    for (uint64_t j = 0; j < std::max(G, M); ++j) {

        pp::placeEntry(q, j, out.grp_prob.data(), out.path_idx.data());
    }

    uint64_t sum = 0;

    for (uint64_t p = 0; p <= P; ++p) {

        const uint64_t length = out.name_off[p];
        out.name_off[p] = sum;
        sum += length;
    }

    if (sum != sink.name_bytes) {

        throw std::runtime_error("the bytes of the names: the sum of the lengths is not the sink's");
    }

    out.name_bytes.resize(sum);

    for (uint64_t b = 0; b < sum; ++b) {

        out.name_bytes[b] = pp::nameByte(text, out.name_off.data(), name_src.data(), P, b);
    }

    return out;
}

template <typename Make>
void * guarded(Make make) {

    try {

        const auto start = std::chrono::steady_clock::now();
        std::unique_ptr<FlatDump> out(new FlatDump(make()));
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        if (out->seconds == 0) out->seconds = seconds;
        return out.release();

    } catch (const std::exception & e) {

        parse_last_error = e.what();
        return nullptr;
    }
}

}

extern "C" {

// flat arrays of a parsed dump; name_bytes is not terminated
struct rpvg_amd_rows_parse_view {

    uint64_t num_clusters, num_paths, num_rows, num_groups, num_entries, num_name_bytes;
    const uint64_t * cluster_row_off, * cluster_path_off, * row_grp_off, * grp_idx_off, * name_off, * num_align_lists, * cluster_index;
    const uint32_t * row_count, * path_idx, * path_length;
    const double * row_noise, * grp_prob, * path_effective_length;
    const uint8_t * has_rank_key;
    const char * name_bytes;
    double seconds;  // of the reader alone (the flattening of containers is outside it where the reader makes containers)
};

const char * rpvg_amd_rows_parse_last_error(void) {

    return parse_last_error.c_str();
}

void * rpvg_amd_rows_parse(void * engine, const char * text, uint64_t num_bytes, double prob_precision) {

    return guarded([&]() {

        const ParsedDump dump(static_cast<Engine *>(engine)->hip, text, num_bytes, false, prob_precision);
        return flatten(dump);
    });
}

void * rpvg_amd_rows_parse_host_line(const char * text, uint64_t num_bytes, double prob_precision) {

    return guarded([&]() {

        const std::string copy(text ? text : "", num_bytes);
        const auto start = std::chrono::steady_clock::now();
        const auto clusters = readProbabilityClustersText(copy, "text", prob_precision);
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        FlatDump out = flatten(clusters);
        out.seconds = seconds;
        return out;
    });
}

void * rpvg_amd_rows_parse_plan(const char * text, uint64_t num_bytes, uint64_t * exact_tokens_out) {

    return guarded([&]() { return planParse(text ? text : "", num_bytes, exact_tokens_out); });
}

// on_device != 0: readProbabilityClustersDevice on the engine; 0: readProbabilityClusters (engine may be NULL)
void * rpvg_amd_rows_parse_file(void * engine, const char * filename, double prob_precision, int on_device) {

    return guarded([&]() {

        return flatten(on_device ? readProbabilityClustersDevice(static_cast<Engine *>(engine)->hip, filename, prob_precision) : readProbabilityClusters(filename, prob_precision));
    });
}

// the seconds readTextFile takes on the file (and the bytes it read), -1 on failure
double rpvg_amd_read_text_file_seconds(const char * filename, uint64_t * bytes_out) {

    try {

        const auto start = std::chrono::steady_clock::now();
        const std::string text = readTextFile(filename);
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();

        if (bytes_out) {

            *bytes_out = text.size();
        }

        return seconds;

    } catch (const std::exception & e) {

        parse_last_error = e.what();
        return -1;
    }
}

int rpvg_amd_rows_parse_view(const void * handle, rpvg_amd_rows_parse_view * view) {

    const FlatDump & d = *static_cast<const FlatDump *>(handle);
    view->num_clusters = d.has_rank_key.size();
    view->num_paths = d.path_length.size();
    view->num_rows = d.row_count.size();
    view->num_groups = d.grp_prob.size();
    view->num_entries = d.path_idx.size();
    view->num_name_bytes = d.name_bytes.size();
    view->cluster_row_off = d.cluster_row_off.data();
    view->cluster_path_off = d.cluster_path_off.data();
    view->row_grp_off = d.row_grp_off.data();
    view->grp_idx_off = d.grp_idx_off.data();
    view->name_off = d.name_off.data();
    view->num_align_lists = d.num_align_lists.data();
    view->cluster_index = d.cluster_index.data();
    view->row_count = d.row_count.data();
    view->path_idx = d.path_idx.data();
    view->path_length = d.path_length.data();
    view->row_noise = d.row_noise.data();
    view->grp_prob = d.grp_prob.data();
    view->path_effective_length = d.path_effective_length.data();
    view->has_rank_key = d.has_rank_key.data();
    view->name_bytes = d.name_bytes.data();
    view->seconds = d.seconds;
    return 0;
}

void rpvg_amd_rows_parse_free(void * handle) {

    delete static_cast<FlatDump *>(handle);
}

}
