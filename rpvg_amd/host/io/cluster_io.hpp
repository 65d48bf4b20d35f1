// On-disk formats on the input side of the inference hot path:
//   <prefix>_probs.txt[.gz]  the dump of the hot-path input written by `--write-probs`
//                            (ProbabilityClusterWriter, src/threaded_output_writer.cpp:42-95)
//   -f path info TSV         Name / Length / Transcript / [Reference] / Haplotypes
//                            (parseHaplotypeTranscriptInfo, src/main.cpp:239-353)
// so that a real rpvg run can be replayed through the GPU engine.  Plain or gzip (zlib).
#ifndef RPVG_AMD_CLUSTER_IO_HPP
#define RPVG_AMD_CLUSTER_IO_HPP

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/rpvg_hip.h"
#include "../../../include/rpvg_text.h"
#include "../path_cluster_estimates.hpp"
#include "../read_path_probabilities.hpp"

namespace rpvg_amd {

// One block of the dump: the cluster's paths (name, length, effective length; local index = position)
// and its merged read rows.
struct ProbabilityCluster {

    std::vector<PathInfo> paths;
    std::vector<ReadPathProbabilities> cluster_probs;

    // What the reference ranks clusters by (src/main.cpp:811-827: descending (number of alignment-path lists, index of the
    // cluster in PathClusters); the rank is the output ClusterID and the offset of the cluster's random seed, :849,976).
    // The reference's dump does not hold them; a producer that knows them writes "# <lists> <index>" as the marker line of
    // the block instead of "#" (has_rank_key).  Without them a replay ranks by read count.
    bool has_rank_key = false;
    uint64_t num_align_lists = 0;
    uint64_t cluster_index = 0;
};

// Text file helpers (zlib): reading passes plain files through; writing gzips when the name ends in ".gz".
std::string readTextFile(const std::string & filename);
void writeTextFile(const std::string & filename, const std::string & text);

// bytes that are a file already (BGZF members): no gzip, whatever the name ends in
void writeRawFile(const std::string & filename, const char * data, const size_t size);

std::vector<ProbabilityCluster> readProbabilityClusters(const std::string & filename, const double prob_precision);

// ... of a text that is in memory already; `source_name` is what the messages of a refused text start with
std::vector<ProbabilityCluster> readProbabilityClustersText(const std::string & text, const std::string & source_name, const double prob_precision);

class HipEngine;

// A dump parsed on the GPU (rpvg_amd/csrc/rows_parse.hip): the resident rows and the path side, without any container.  The
// handle of the C ABI behind a class; a refused text throws std::runtime_error with the line and the reason.
class ParsedDump {

    public:

        // bytes: host memory, or device memory of the engine's GPU (on_device)
        ParsedDump(const std::shared_ptr<HipEngine> & engine, const char * bytes, const uint64_t num_bytes, const bool on_device, const double prob_precision);
        ~ParsedDump();

        ParsedDump(const ParsedDump &) = delete;
        ParsedDump & operator=(const ParsedDump &) = delete;

        rpvg_hip_parsed_dump * handle() const { return dump; }
        rpvg_hip_read_rows * rows() const { return rpvg_hip_parsed_dump_rows(dump); }

        // host copies, valid until the dump dies
        rpvg_parsed_dump_view view() const;
        rpvg_cluster_batch rowsView() const;

        // the names, lengths and ClusterIDs where they lie on the GPU
        rpvg_table_labels labels() const;

        // the batch the estimators take, made on the GPU from the resident rows (the caller's, rpvg_hip_batch_free)
        rpvg_hip_batch * toBatch() const;

    private:

        std::shared_ptr<HipEngine> hip_engine;
        rpvg_hip_parsed_dump * dump = nullptr;
};

// readProbabilityClusters through the device parse: readTextFile, the kernels, then the same containers from the views.  For
// callers that want the containers; the device refuses some texts std::stod takes ("1.5abc", "0x1p3", "+1", a space at the end
// of a line: docs/design/parity.md item 22), for which readProbabilityClusters stays.
std::vector<ProbabilityCluster> readProbabilityClustersDevice(const std::shared_ptr<HipEngine> & engine, const std::string & filename, const double prob_precision);
std::vector<ProbabilityCluster> readProbabilityClustersDeviceText(const std::shared_ptr<HipEngine> & engine, const std::string & text, const double prob_precision);

// Same format as the reference's writer (a block whose cluster has a rank key gets the extended marker line); gzip when the
// name ends in ".gz".
void writeProbabilityClusters(const std::string & filename, const std::vector<ProbabilityCluster> & clusters, const double prob_precision);

// ... its text, without the file
std::string formatProbabilityClusters(const std::vector<ProbabilityCluster> & clusters, const double prob_precision);

// The same file from a text formatted on the GPU (TableText::rows, table_text.hpp): the block goes into the file as it is.
void writeProbabilityClustersText(const std::string & filename, const rpvg_table_text_view & text);

// The same file from the BGZF members the GPU deflated that text into (TableText::bgzf): the members as they are, then BGZF's
// end-of-file block.  A gzip reader gives the bytes of the text.
void writeProbabilityClustersBgzf(const std::string & filename, const rpvg_text_bgzf_view & members);

// Path name -> PathInfo with group_id (dense transcript ids in first-seen order), source_count and — when
// parse_haplotype_ids — source_ids (dense haplotype ids in first-seen order); use_transcript_names
// replaces the name by the transcript's (the reference does that when collapsing haplotypes).
std::unordered_map<std::string, PathInfo> parseHaplotypeTranscriptInfo(const std::string & filename, const bool parse_haplotype_ids, const bool use_transcript_names);

// Fills group_id / source_count / source_ids of the clusters' paths from the info by path name
// (src/main.cpp:866-872).  Throws std::runtime_error when a path is missing from the info.
void applyHaplotypeTranscriptInfo(std::vector<ProbabilityCluster> * clusters, const std::unordered_map<std::string, PathInfo> & haplotype_transcript_info);

}

#endif
