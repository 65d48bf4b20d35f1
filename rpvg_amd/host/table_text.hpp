// The rows of a result file as text, formatted on the GPU from a resident table (include/rpvg_text.h, rpvg_amd/csrc/table_text.hip):
// the rows of ReadCountGibbsSamplesWriter, AbundanceEstimatesWriter and HaplotypeAbundanceEstimatesWriter
// (src/threaded_output_writer.cpp:160-201, :295-322, :358-411) as one block of bytes, which the writers' addText()
// (io/estimates_writers.hpp) append as they are.  Nothing here formats: FlatLabels flattens TableLabels, TableText forwards to the
// GPU and holds the view.  hostLine() is the comparison line: the same row descriptors (rpvg_amd/csrc/table_text_plan.hpp) walked on
// one host thread, for the timing of tools/table_text_ab.py and for the CPU checks.
#ifndef RPVG_AMD_TABLE_TEXT_HPP
#define RPVG_AMD_TABLE_TEXT_HPP

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rpvg_text.h"
#include "../csrc/rows_text_plan.hpp"
#include "../csrc/set_text_plan.hpp"
#include "../csrc/table_text_plan.hpp"
#include "estimates_table.hpp"
#include "gibbs_samples_table.hpp"
#include "hip_engine.hpp"
#include "io/cluster_io.hpp"
#include "io/estimates_writers.hpp"

namespace rpvg_amd {

// TableLabels in the flat form of rpvg_table_labels (host memory)
struct FlatLabels {

    std::vector<uint64_t> name_off;
    std::string name_bytes;
    std::vector<uint32_t> lengths, cluster_ids;

    explicit FlatLabels(const TableLabels & labels) : name_off(1, 0), lengths(labels.lengths), cluster_ids(labels.cluster_ids) {

        for (auto & name: labels.names) {

            name_bytes += name;
            name_off.push_back(name_bytes.size());
        }
    }

    // valid while this lives
    rpvg_table_labels view() const {

        rpvg_table_labels flat = {};
        flat.num_clusters = cluster_ids.size();
        flat.num_paths = name_off.size() - 1;
        flat.num_name_bytes = name_bytes.size();
        flat.name_off = name_off.data();
        flat.name_bytes = name_bytes.data();
        flat.path_length = lengths.size() == flat.num_paths ? lengths.data() : nullptr;
        flat.cluster_id = cluster_ids.data();
        flat.on_device = 0;

        return flat;
    }
};

// The rows and paths of a --write-probs dump in the flat form of rpvg_rows_text_input and rpvg_table_labels (host memory): a copy of
// such arrays, or the clusters of the writer (io/cluster_io.hpp) flattened.
struct FlatRows {

    std::vector<uint64_t> cluster_row_off, cluster_path_off, row_grp_off, grp_idx_off, num_align_lists, cluster_index, name_off;
    std::vector<uint32_t> row_count, path_idx, path_length;
    std::vector<double> row_noise, grp_prob, path_effective_length;
    std::string name_bytes;

    // host pointers; the sizes are the input's
    FlatRows(const rpvg_rows_text_input & in, const rpvg_table_labels & labels) {

        const size_t K = in.num_clusters, R = in.num_rows, G = in.num_groups, M = in.num_entries, P = in.num_paths;

        if (in.on_device || labels.on_device || labels.num_paths != P || (P && !labels.path_length)) {

            throw std::runtime_error("FlatRows: host arrays and labels with path_length of the input's paths");
        }

        const auto copy = [](auto & into, const auto * from, const size_t n) { if (from) into.assign(from, from + n); };
        copy(cluster_row_off, in.cluster_row_off, K + 1);
        copy(cluster_path_off, in.cluster_path_off, K + 1);
        copy(row_count, in.row_count, R);
        copy(row_noise, in.row_noise, R);
        copy(row_grp_off, in.row_grp_off, R + 1);
        copy(grp_prob, in.grp_prob, G);
        copy(grp_idx_off, in.grp_idx_off, G + 1);
        copy(path_idx, in.path_idx, M);
        copy(path_effective_length, in.path_effective_length, P);
        copy(num_align_lists, in.num_align_lists, K);
        copy(cluster_index, in.cluster_index, K);
        copy(name_off, labels.name_off, P + 1);
        copy(path_length, labels.path_length, P);
        copy(name_bytes, labels.name_bytes, labels.num_name_bytes);
        has_rank_keys = in.num_align_lists && in.cluster_index;
    }

    // rank keys in the markers iff every cluster has one (an empty list: none)
    explicit FlatRows(const std::vector<ProbabilityCluster> & clusters) : cluster_row_off(1, 0), cluster_path_off(1, 0), row_grp_off(1, 0), grp_idx_off(1, 0), name_off(1, 0) {

        has_rank_keys = !clusters.empty();

        for (auto & cluster: clusters) {

            has_rank_keys = has_rank_keys && cluster.has_rank_key;
            num_align_lists.emplace_back(cluster.num_align_lists);
            cluster_index.emplace_back(cluster.cluster_index);

            for (auto & path: cluster.paths) {

                name_bytes += path.name;
                name_off.emplace_back(name_bytes.size());
                path_length.emplace_back(path.length);
                path_effective_length.emplace_back(path.effective_length);
            }

            for (auto & read_path_probs: cluster.cluster_probs) {

                row_count.emplace_back(read_path_probs.readCount());
                row_noise.emplace_back(read_path_probs.noiseProb());

                for (auto & path_probs: read_path_probs.pathProbs()) {

                    grp_prob.emplace_back(path_probs.first);
                    path_idx.insert(path_idx.end(), path_probs.second.begin(), path_probs.second.end());
                    grp_idx_off.emplace_back(path_idx.size());
                }

                row_grp_off.emplace_back(grp_prob.size());
            }

            cluster_row_off.emplace_back(row_count.size());
            cluster_path_off.emplace_back(path_length.size());
        }
    }

    // valid while this lives
    rpvg_rows_text_input input() const {

        rpvg_rows_text_input in = {};
        in.num_clusters = cluster_row_off.empty() ? 0 : cluster_row_off.size() - 1;
        in.num_rows = row_count.size();
        in.num_groups = grp_prob.size();
        in.num_entries = path_idx.size();
        in.num_paths = path_length.size();
        in.cluster_row_off = cluster_row_off.data();
        in.cluster_path_off = cluster_path_off.data();
        in.row_count = row_count.data();
        in.row_noise = row_noise.data();
        in.row_grp_off = row_grp_off.data();
        in.grp_prob = grp_prob.data();
        in.grp_idx_off = grp_idx_off.data();
        in.path_idx = path_idx.data();
        in.path_effective_length = path_effective_length.data();
        in.num_align_lists = has_rank_keys ? num_align_lists.data() : nullptr;
        in.cluster_index = has_rank_keys ? cluster_index.data() : nullptr;

        return in;
    }

    // (cluster_id is not read by the dump)
    rpvg_table_labels labels() const {

        rpvg_table_labels flat = {};
        flat.num_clusters = cluster_row_off.empty() ? 0 : cluster_row_off.size() - 1;
        flat.num_paths = path_length.size();
        flat.num_name_bytes = name_bytes.size();
        flat.name_off = name_off.data();
        flat.name_bytes = name_bytes.data();
        flat.path_length = path_length.data();

        return flat;
    }

    bool has_rank_keys = false;
};

class TableText {

    public:

        // the rows ReadCountGibbsSamplesWriter::addTable prints from the table
        TableText(std::shared_ptr<HipEngine> engine_in, GibbsSamplesTable & table, const int32_t precision) : hip_engine(std::move(engine_in)), text(nullptr), text_view(), has_view(false) {

            const FlatLabels labels(table.labels());
            const rpvg_table_labels flat = labels.view();
            HipEngine::check(rpvg_hip_gibbs_table_text(hip_engine->ctx(), table.handle(), &flat, precision, &text), "rpvg_hip_gibbs_table_text");
        }

        // kind RPVG_TEXT_PER_PATH: the rows of AbundanceEstimatesWriter::addTable; RPVG_TEXT_HAPLOTYPE: those of
        // HaplotypeAbundanceEstimatesWriter::addTable.  After EstimatesTable::tpm().
        TableText(std::shared_ptr<HipEngine> engine_in, EstimatesTable & table, const TableLabels & table_labels, const int32_t kind, const int32_t precision) : hip_engine(std::move(engine_in)), text(nullptr), text_view(), has_view(false) {

            const FlatLabels labels(table_labels);
            const rpvg_table_labels flat = labels.view();
            const rpvg_estimates_flat estimates = table.deviceEstimates();
            HipEngine::check(rpvg_hip_estimates_table_text(hip_engine->ctx(), table.handle(), &estimates, &flat, kind, precision, &text), "rpvg_hip_estimates_table_text");
        }

        // The rows whose unit is a path group set.  kind RPVG_TEXT_JOINT: the rows of JointHaplotypeAbundanceEstimatesWriter::addTable,
        // after EstimatesTable::tpm(), from a table built for `ploidy`; RPVG_TEXT_POSTERIOR: the rows of
        // JointHaplotypeEstimatesWriter::addTable, which need neither abundances nor TPMs.  In the view num_paths is the number of sets.
        static std::unique_ptr<TableText> sets(std::shared_ptr<HipEngine> engine_in, EstimatesTable & table, const TableLabels & table_labels, const int32_t kind, const uint32_t ploidy, const double min_posterior, const int32_t precision) {

            std::unique_ptr<TableText> out(new TableText(std::move(engine_in)));
            const FlatLabels labels(table_labels);
            const rpvg_table_labels flat = labels.view();
            const rpvg_estimates_flat estimates = table.deviceEstimates();
            HipEngine::check(rpvg_hip_estimates_set_text(out->hip_engine->ctx(), table.handle(), &estimates, &flat, kind, ploidy, min_posterior, precision, &out->text), "rpvg_hip_estimates_set_text");

            return out;
        }

        // The --write-probs dump (ProbabilityClusterWriter::addCluster, src/threaded_output_writer.cpp:40-95) of flat rows, host or
        // device arrays: in the view the rows are the 2 K + R lines of the text.  writeProbabilityClustersText (io/cluster_io.hpp)
        // puts the view into the file.
        static std::unique_ptr<TableText> rows(std::shared_ptr<HipEngine> engine_in, const rpvg_rows_text_input & input, const rpvg_table_labels & labels, const double prob_precision) {

            std::unique_ptr<TableText> out(new TableText(std::move(engine_in)));
            HipEngine::check(rpvg_hip_rows_text(out->hip_engine->ctx(), &input, &labels, prob_precision, &out->text), "rpvg_hip_rows_text");

            return out;
        }

        // ... of the writer's clusters, flattened
        static std::unique_ptr<TableText> rows(std::shared_ptr<HipEngine> engine_in, const std::vector<ProbabilityCluster> & clusters, const double prob_precision) {

            const FlatRows flat(clusters);

            return rows(std::move(engine_in), flat.input(), flat.labels(), prob_precision);
        }

        // ... of resident rows (rpvg_hip_read_rows_build), read where they lie; labels and effective lengths of the rows' columns
        static std::unique_ptr<TableText> rows(std::shared_ptr<HipEngine> engine_in, const rpvg_hip_read_rows * resident, const rpvg_table_labels & labels, const double * path_effective_length, const uint64_t * num_align_lists, const uint64_t * cluster_index, const double prob_precision) {

            std::unique_ptr<TableText> out(new TableText(std::move(engine_in)));
            HipEngine::check(rpvg_hip_read_rows_text(out->hip_engine->ctx(), resident, &labels, path_effective_length, num_align_lists, cluster_index, prob_precision, &out->text), "rpvg_hip_read_rows_text");

            return out;
        }

        ~TableText() {

            rpvg_hip_text_bgzf_free(members);
            rpvg_hip_table_text_free(text);
        }

        TableText(const TableText &) = delete;
        TableText & operator=(const TableText &) = delete;

        // row_off and one page-locked copy of the whole text; valid until the text's end
        const rpvg_table_text_view & view() {

            if (!has_view) {

                HipEngine::check(rpvg_hip_table_text_view(text, &text_view), "rpvg_hip_table_text_view");
                has_view = true;
            }

            return text_view;
        }

        // the sizes and row_off without the copy of the text (bytes is NULL unless view() has run): for a writer that takes bgzf()
        rpvg_table_text_view sizes() {

            rpvg_table_text_view out = {};
            HipEngine::check(rpvg_hip_table_text_sizes(text, &out), "rpvg_hip_table_text_sizes");

            return out;
        }

        // bytes [begin, end) only, for a writer that streams a text it could not hold twice
        std::string bytes(const uint64_t begin, const uint64_t end) {

            std::string out(end > begin ? end - begin : 0, '\0');
            HipEngine::check(rpvg_hip_table_text_get(text, begin, end, out.empty() ? nullptr : &out[0]), "rpvg_hip_table_text_get");

            return out;
        }

        // The text as BGZF members, deflated on the GPU on the first call (rpvg_amd/csrc/text_deflate.hip): the sizes, member_off and
        // one page-locked copy of the compressed bytes, which ReadCountGibbsSamplesWriter::addCompressedText and
        // writeProbabilityClustersBgzf put into the .gz file.  The plain text need not be downloaded for it.  Valid until the text's end.
        const rpvg_text_bgzf_view & bgzf() {

            deflate();

            if (!has_members_view) {

                HipEngine::check(rpvg_hip_text_bgzf_view(members, &members_view), "rpvg_hip_text_bgzf_view");
                has_members_view = true;
            }

            return members_view;
        }

        // the first half of bgzf() alone: the members are made and stay on the GPU
        void deflate() {

            if (!members) {

                HipEngine::check(rpvg_hip_table_text_bgzf(text, &members), "rpvg_hip_table_text_bgzf");
            }
        }

    private:

        explicit TableText(std::shared_ptr<HipEngine> engine_in) : hip_engine(std::move(engine_in)), text(nullptr), text_view(), has_view(false) {}

        std::shared_ptr<HipEngine> hip_engine;
        rpvg_hip_table_text * text;
        rpvg_table_text_view text_view;
        bool has_view;
        rpvg_hip_text_bgzf * members = nullptr;
        rpvg_text_bgzf_view members_view = {};
        bool has_members_view = false;
};

// ---- the comparison line: the same rows on one host thread ----------------------------------------------------------------------

struct HostLine {

    std::vector<uint64_t> row_off;
    std::string bytes;
    uint64_t exact_cells = 0;
};

inline const uint64_t * hostPow10Table() {

    static const std::vector<uint64_t> words = [] {

        std::vector<uint64_t> table(rpvg_number_text::kPow10Words);
        rpvg_number_text::buildPow10Table(table.data(), nullptr);
        return table;
    }();

    return words.data();
}

// the descriptor of the Gibbs rows over the host view of the table
inline rpvg_table_text::TextRows gibbsTextRows(const rpvg_gibbs_table_view & table, const rpvg_table_labels & labels, const int32_t precision) {

    rpvg_table_text::TextRows rows = {};
    rows.num_rows = table.num_paths;
    rows.num_clusters = table.num_clusters;
    rows.name_off = labels.name_off;
    rows.name_bytes = labels.name_bytes;
    rows.cluster_path_off = table.cluster_path_off;
    rows.cluster_id = labels.cluster_id;
    rows.run_length = table.num_gibbs_samples;
    rows.run = table.samples;
    rows.run_stride = table.num_gibbs_samples;
    rows.filter = table.listed;
    rows.precision = precision;
    rows.pow10 = hostPow10Table();

    return rows;
}

// the descriptor of the estimates rows over the host estimates and the host view of the table; member_base is filled for the
// per-path kind and must outlive the descriptor (set i = {i} is the caller's precondition, as it is addTable()'s)
inline rpvg_table_text::TextRows estimatesTextRows(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const rpvg_table_labels & labels, const int32_t kind, const int32_t precision, std::vector<uint64_t> * member_base) {

    rpvg_table_text::TextRows rows = {};
    rows.num_rows = table.num_paths;
    rows.num_clusters = table.num_clusters;
    rows.name_off = labels.name_off;
    rows.name_bytes = labels.name_bytes;
    rows.cluster_path_off = estimates.cluster_path_off;
    rows.cluster_id = labels.cluster_id;
    rows.second_u32 = labels.path_length;
    rows.precision = precision;
    rows.pow10 = hostPow10Table();
    rows.fixed[0] = rpvg_table_text::DoubleColumn{estimates.path_effective_length, nullptr};

    if (kind == RPVG_TEXT_PER_PATH) {

        member_base->assign(table.num_clusters, 0);

        for (uint32_t k = 0; k < table.num_clusters; ++k) {

            (*member_base)[k] = estimates.member_off[estimates.set_off[k]];
        }

        rows.num_fixed = 3;
        rows.fixed[1] = rpvg_table_text::DoubleColumn{estimates.abundances, estimates.abund_off};
        rows.fixed[2] = rpvg_table_text::DoubleColumn{table.member_tpm, member_base->data()};

    } else {

        rows.num_fixed = 4;
        rows.fixed[1] = rpvg_table_text::DoubleColumn{table.haplotype_prob, nullptr};
        rows.fixed[2] = rpvg_table_text::DoubleColumn{table.read_count, nullptr};
        rows.fixed[3] = rpvg_table_text::DoubleColumn{table.tpm, nullptr};
    }

    return rows;
}

inline HostLine hostLine(const rpvg_table_text::TextRows & rows) {

    if (const char * wrong = rpvg_table_text::descriptorBad(rows)) {

        throw std::runtime_error(std::string("hostLine: ") + wrong);
    }

    HostLine line;
    line.row_off.assign(rows.num_rows + 1, 0);

    for (uint64_t r = 0; r < rows.num_rows; ++r) {

        line.row_off[r + 1] = line.row_off[r] + rpvg_table_text::rowBytes(rows, r, &line.exact_cells);
    }

    line.bytes.assign(line.row_off[rows.num_rows], '\0');

    for (uint64_t r = 0; r < rows.num_rows; ++r) {

        rpvg_table_text::rowWrite(rows, r, &line.bytes[line.row_off[r]]);
    }

    return line;
}

// the descriptor of the set rows over the host estimates and the host view of the table (which the posterior kind does not read)
inline rpvg_set_text::SetRows setsTextRows(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const rpvg_table_labels & labels, const int32_t kind, const uint32_t ploidy, const double min_posterior, const int32_t precision) {

    const bool joint = kind == RPVG_TEXT_JOINT;

    rpvg_set_text::SetRows rows = {};
    rows.num_sets = estimates.num_sets;
    rows.num_clusters = estimates.num_clusters;
    rows.ploidy = ploidy;
    rows.joint = joint;
    rows.name_off = labels.name_off;
    rows.name_bytes = labels.name_bytes;
    rows.cluster_path_off = estimates.cluster_path_off;
    rows.cluster_id = labels.cluster_id;
    rows.set_off = estimates.set_off;
    rows.member_off = estimates.member_off;
    rows.members = estimates.members;
    rows.posteriors = estimates.posteriors;
    rows.abund_off = joint ? estimates.abund_off : nullptr;
    rows.abundances = joint ? estimates.abundances : nullptr;
    rows.member_tpm = joint ? table.member_tpm : nullptr;
    rows.min_posterior = min_posterior;
    rows.precision = precision;
    rows.pow10 = hostPow10Table();

    return rows;
}

// the comparison line of the set rows (valid sets are the caller's precondition, as they are addTable()'s)
inline HostLine hostLineSets(const rpvg_set_text::SetRows & rows) {

    if (const char * wrong = rpvg_set_text::descriptorBad(rows)) {

        throw std::runtime_error(std::string("hostLineSets: ") + wrong);
    }

    HostLine line;
    line.row_off.assign(rows.num_sets + 1, 0);

    for (uint64_t s = 0; s < rows.num_sets; ++s) {

        line.row_off[s + 1] = line.row_off[s] + rpvg_set_text::rowBytes(rows, s, &line.exact_cells);
    }

    line.bytes.assign(line.row_off[rows.num_sets], '\0');

    for (uint64_t s = 0; s < rows.num_sets; ++s) {

        rpvg_set_text::rowWrite(rows, s, &line.bytes[line.row_off[s]]);
    }

    return line;
}

// the descriptor of the dump over host arrays (prob_precision in (0, 1) and at most 17 digits are the caller's precondition)
inline rpvg_rows_text::DumpRows dumpTextRows(const rpvg_rows_text_input & input, const rpvg_table_labels & labels, const double prob_precision) {

    if (const char * wrong = rpvg_rows_text::probPrecisionBad(prob_precision)) {

        throw std::runtime_error(std::string("dumpTextRows: ") + wrong);
    }

    rpvg_rows_text::DumpRows rows = {};
    rows.num_clusters = input.num_clusters;
    rows.num_rows = input.num_rows;
    rows.num_groups = input.num_groups;
    rows.num_entries = input.num_entries;
    rows.num_paths = input.num_paths;
    rows.cluster_row_off = input.cluster_row_off;
    rows.cluster_path_off = input.cluster_path_off;
    rows.row_count = input.row_count;
    rows.row_noise = input.row_noise;
    rows.row_grp_off = input.row_grp_off;
    rows.grp_prob = input.grp_prob;
    rows.grp_idx_off = input.grp_idx_off;
    rows.path_idx = input.path_idx;
    rows.name_off = labels.name_off;
    rows.name_bytes = labels.name_bytes;
    rows.path_length = labels.path_length;
    rows.path_effective_length = input.path_effective_length;
    rows.num_align_lists = input.num_align_lists;
    rows.cluster_index = input.cluster_index;
    rows.digits = rpvg_rows_text::probPrecisionDigits(prob_precision);
    rows.pow10 = hostPow10Table();

    return rows;
}

// the comparison line of the dump: rowWrite walked on one thread (valid offsets and indices are the caller's precondition); the rows
// of the line are the 2 K + R lines of the text
inline HostLine hostLineRows(const rpvg_rows_text::DumpRows & rows) {

    if (const char * wrong = rpvg_rows_text::descriptorBad(rows)) {

        throw std::runtime_error(std::string("hostLineRows: ") + wrong);
    }

    const uint64_t num_lines = rpvg_rows_text::numLines(rows);
    HostLine line;
    line.row_off.assign(num_lines + 1, 0);

    for (uint64_t j = 0; j < num_lines; ++j) {

        line.row_off[j + 1] = line.row_off[j] + rpvg_rows_text::rowBytes(rows, j, &line.exact_cells);
    }

    line.bytes.assign(line.row_off[num_lines], '\0');

    for (uint64_t j = 0; j < num_lines; ++j) {

        rpvg_rows_text::rowWrite(rows, j, &line.bytes[line.row_off[j]]);
    }

    return line;
}

}

#endif
