// Result files on the output side of the inference hot path, in the formats of the reference's
// writers (src/threaded_output_writer.{hpp,cpp}): tab-separated, std::setprecision(8) default float
// formatting, one `Unknown` row carrying the noise read count.
//
//   AbundanceEstimatesWriter                 <prefix>.txt        -i transcripts / strains      :283-343
//   HaplotypeAbundanceEstimatesWriter        <prefix>.txt        -i haplotype-transcripts      :346-432
//   JointHaplotypeAbundanceEstimatesWriter   <prefix>_joint.txt  -i haplotype-transcripts      :434-546
//   JointHaplotypeEstimatesWriter            <prefix>.txt        -i haplotypes                 :233-280
//   ReadCountGibbsSamplesWriter              <prefix>_gibbs.txt.gz  -n > 0                     :98-230
//
// The reference streams string buffers to a BGZF writer thread; these writers collect the text and write
// the file on close() (plain text, gzip for the ".gz" one; BGZF members from the GPU as they are).  Row order across clusters follows the order
// of the addEstimates() calls (the reference's order depends on its OpenMP schedule).
#ifndef RPVG_AMD_ESTIMATES_WRITERS_HPP
#define RPVG_AMD_ESTIMATES_WRITERS_HPP

#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/rpvg_table.h"
#include "../../../include/rpvg_samples.h"
#include "../../../include/rpvg_text.h"
#include "../path_cluster_estimates.hpp"

namespace rpvg_amd {

typedef std::vector<std::pair<uint32_t, PathClusterEstimates> > ClusterEstimatesList;

// Sum of abundance / effective length over every group-set member of every cluster
// (src/main.cpp:1029-1057): the TPM denominator.
double totalTranscriptCount(const ClusterEstimatesList & path_cluster_estimates);

// What the rows of an estimates table (include/rpvg_table.h) are called: name and length of every path of the batch in cluster
// order (the batch-wide slots of the table), and the ClusterID of every cluster.
struct TableLabels {

    std::vector<std::string> names;
    std::vector<uint32_t> lengths;
    std::vector<uint32_t> cluster_ids;
};

class EstimatesWriter {

    public:

        explicit EstimatesWriter(const std::string & filename_in);
        virtual ~EstimatesWriter() {};

        void close();

    protected:

        std::stringstream out;

        // A writer that took members the GPU deflated (rpvg_amd/csrc/text_deflate.hip): what the stream holds so far becomes members
        // framed on the host (rpvg_amd/csrc/text_deflate_plan.hpp), the device's members follow as they are.  close() then frames
        // the rest of the stream, appends BGZF's end-of-file block and writes the bytes as they are.
        void appendMembers(const rpvg_text_bgzf_view & members);

    private:

        void frameStream();

        const std::string filename;
        std::string framed;
        bool has_members = false;
};

class AbundanceEstimatesWriter : public EstimatesWriter {

    public:

        AbundanceEstimatesWriter(const std::string filename_prefix, const double total_transcript_count_in);

        void addEstimates(const ClusterEstimatesList & path_cluster_estimates);
        void addNoiseTranscript(const uint32_t unaligned_read_count);

        // The same rows from the table the GPU built of the estimates (rpvg_amd/host/estimates_table.hpp) and the flat estimates
        // it was built from, after EstimatesTable::tpm(): for a denominator > 0 the text is what addEstimates() writes from the
        // containers, byte for byte — the rows always, the `Unknown` row for ONE table per writer: the table's noise total joins the
        // writer's in one addition, where addEstimates() adds cluster by cluster onto the running value, so with several batches
        // into one writer the noise of the `Unknown` row can differ in its last digit.  Throws EngineError for a table without TPMs or labels of another size, and for a cluster
        // whose set i is not {i} (what addEstimates() asserts).
        void addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels);

        // The rows as text the GPU formatted from the table (rpvg_amd/host/table_text.hpp): the writer's noise total moves on exactly as
        // in addTable(), then the block is appended to the stream as it is.  Throws EngineError for a table without TPMs or a text
        // of another number of paths.
        void addText(const rpvg_estimates_table_view & table, const rpvg_table_text_view & text);

    private:

        const double total_transcript_count;
        double noise_count;
};

class HaplotypeAbundanceEstimatesWriter : public EstimatesWriter {

    public:

        HaplotypeAbundanceEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double total_transcript_count_in);

        void addEstimates(const ClusterEstimatesList & path_cluster_estimates);
        void addNoiseTranscript(const uint32_t unaligned_read_count);

        // The same rows from the table the GPU built of the estimates (rpvg_amd/host/estimates_table.hpp) and the flat estimates
        // it was built from, after EstimatesTable::tpm(): for a denominator > 0 the text is what addEstimates() writes from the
        // containers, byte for byte — the rows always, the `Unknown` row for ONE table per writer: the table's noise total joins the
        // writer's in one addition, where addEstimates() adds cluster by cluster onto the running value, so with several batches
        // into one writer the noise of the `Unknown` row can differ in its last digit.  Throws EngineError for a table without TPMs or labels of another size.
        void addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels);

        // The rows as text the GPU formatted from the table (rpvg_amd/host/table_text.hpp): the writer's noise total moves on exactly as
        // in addTable(), then the block is appended to the stream as it is.  Throws EngineError for a table without TPMs or a text
        // of another number of paths.
        void addText(const rpvg_estimates_table_view & table, const rpvg_table_text_view & text);

    private:

        const uint32_t ploidy;
        const double total_transcript_count;
        double noise_count;
};

class JointHaplotypeAbundanceEstimatesWriter : public EstimatesWriter {

    public:

        JointHaplotypeAbundanceEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double min_posterior_in, const double total_transcript_count_in);

        void addEstimates(const ClusterEstimatesList & path_cluster_estimates);
        void addNoiseTranscript(const uint32_t unaligned_read_count);

        // The same rows from the table the GPU built of the estimates (rpvg_amd/host/estimates_table.hpp) and the flat estimates
        // it was built from, after EstimatesTable::tpm(): for a denominator > 0 the text is what addEstimates() writes from the
        // containers, byte for byte — the rows always, the `Unknown` row for ONE table per writer: the table's noise total joins the
        // writer's in one addition, where addEstimates() adds cluster by cluster onto the running value, so with several batches
        // into one writer the noise of the `Unknown` row can differ in its last digit.  Throws EngineError for a table without TPMs or labels of another size, and for a table of
        // another ploidy (its noise share is noise_count / ploidy).
        void addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels);

        // The rows as text the GPU formatted from the table (TableText::sets with RPVG_TEXT_JOINT, this writer's ploidy and
        // min_posterior; rpvg_amd/host/table_text.hpp): the writer's noise shares move on exactly as in addTable(), then the block is
        // appended to the stream as it is.  Throws EngineError for a table without TPMs or of another ploidy and for a text of
        // another number of sets than the estimates'.
        void addText(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text);

    private:

        const uint32_t ploidy;
        const double min_posterior;
        const double total_transcript_count;
        std::vector<double> noise_counts;
};

class JointHaplotypeEstimatesWriter : public EstimatesWriter {

    public:

        JointHaplotypeEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double min_posterior_in);

        void addEstimates(const ClusterEstimatesList & path_cluster_estimates);

        // The same rows from the flat estimates of a batch (host memory) and its labels: the text is what addEstimates() writes
        // from the containers, byte for byte.  A `haplotypes` result has neither abundances nor TPMs and none are read.  Throws
        // EngineError for labels of another size, a set whose size is not in 1 .. ploidy (what addEstimates() asserts) and a set
        // member that is not a path of its cluster.
        void addTable(const rpvg_estimates_flat & estimates, const TableLabels & labels);

        // The rows as text the GPU formatted (TableText::sets with RPVG_TEXT_POSTERIOR, this writer's ploidy and min_posterior):
        // the block is appended to the stream as it is.  Throws EngineError for a text of another number of sets than the estimates'.
        void addText(const rpvg_estimates_flat & estimates, const rpvg_table_text_view & text);

    private:

        const uint32_t ploidy;
        const double min_posterior;
};

class ReadCountGibbsSamplesWriter : public EstimatesWriter {

    public:

        ReadCountGibbsSamplesWriter(const std::string filename_prefix, const uint32_t num_gibbs_samples_in);

        void addSamples(const std::pair<uint32_t, PathClusterEstimates> & path_cluster_estimate);
        void addNoiseTranscript(const uint32_t unaligned_read_count);

        // The same rows from the table the GPU built of the samples of a batch (rpvg_amd/host/gibbs_samples_table.hpp): the listed
        // rows of the view in path order, named by the labels.
        // For ONE table per writer the text is what addSamples() writes cluster by cluster from the containers, byte for byte, the
        // `Unknown` row included: the table's noise_counts are the writer's own chains.  With several tables into one writer a
        // table's noise_counts join the writer's in one addition per column, where addSamples() adds cluster by cluster onto the
        // running values, so the `Unknown` row can then differ in its last digit.  Throws EngineError for a view of another number
        // of samples or labels of another size.
        void addTable(const rpvg_gibbs_table_view & table, const TableLabels & labels);

        // The rows as text the GPU formatted from the table (rpvg_amd/host/table_text.hpp): the table's noise_counts join the writer's
        // exactly as in addTable(), then the block is appended to the stream as it is.  Throws EngineError for a view of another
        // number of samples or a text of another number of paths.
        void addText(const rpvg_gibbs_table_view & table, const rpvg_table_text_view & text);

        // The same text as BGZF members the GPU deflated (TableText::bgzf): addText()'s checks, and the members must be those of the
        // text (num_text_bytes).  The text's bytes are not read, so TableText::sizes() serves and the plain text stays on the GPU.  The file is then the header row as a member framed here, the device's members, the `Unknown` row
        // as a member framed here and the end-of-file block: gzip readers give the bytes of the file addText() leads to.
        void addCompressedText(const rpvg_gibbs_table_view & table, const rpvg_table_text_view & text, const rpvg_text_bgzf_view & members);

    private:

        const uint32_t num_gibbs_samples;
        std::vector<double> noise_counts;
};

}

#endif
