// rows_parse.hip — the --write-probs dump read on the GPU: text bytes in, resident rows (rpvg_hip_read_rows) and the dump's path
// side out (interface include/rpvg_text.h, include/rpvg_hip.h).  The inverse of rows_text.hip; the result is bit for bit what
// readProbabilityClusters makes of the same text.
//
// Takes over   readProbabilityClusters                       rpvg_amd/host/io/cluster_io.cpp:135-251
//              the sort of the ReadPathProbabilities constructor   rpvg_amd/host/read_path_probabilities.cpp:17-21
//
// Work is assigned by byte and by token, never by line: every kernel below is a thread per byte of the text (or per entry of an
// output array) around a function of rows_parse_plan.hpp, which holds the grammar.
//   Flags     rawFlags per byte, then four inclusive max-scans (hipcub, in place): where the byte's line, its field, the last ':'
//             and the last ',' start.
//   Count     countFlags per byte, then five exclusive sums (in place, a trailing 0): the output position of every marker, path
//             field, row, group and index.  Their last entries K, P, R, G, M come back in one page-locked fetch beside the offender
//             word: the first wait.  The arrays get their exact sizes.
//   Fill      markerByte (the clusters' offsets, which the index check reads), then fillByte: the thread of a token's last byte
//             parses and stores it.  One offender word carries the smallest offending line and its reason; the bytes of the names
//             and the tokens decided by the exact comparison are integer sums beside it.  The second wait.
//   Order     a group compares with the one in front of it (orderGroup); a row with a descent is sorted by one thread (sortRow) or,
//             above kMaxUnsortedGroups groups, refused; placeEntry
//             gathers probabilities and indices into the final order.  Rows in order pay the comparison and the copy.
//   Names     name_len summed in place into name_off; a thread per byte of the names (nameByte).
// Memory    nine 32-bit words per byte of text for the scans, the text, and the text-order copies of probabilities and indices beside
//           the final arrays: about 50 bytes per byte of text while a parse runs (the practical limit below the 2^31 - 2 bytes).
// All stores are plain C++ or integer atomics; there is no floating-point arithmetic but the parse's comparisons, so two parses
// give the same bytes.

#include <memory>
#include <mutex>

#include "device_algos.hpp"
#include "read_rows.hpp"
#include "rows_parse_plan.hpp"
#include "rows_text_plan.hpp"
#include "table_kit.hpp"
#include "table_text_device.hpp"
#include "../../include/rpvg_text.h"

using namespace rpvg_hip_detail;
namespace pp = rpvg_rows_parse;

struct rpvg_hip_parsed_dump {
    rpvg_hip_ctx * ctx = nullptr;
    std::unique_ptr<rpvg_hip_read_rows> rows;
    uint32_t num_clusters = 0;
    uint64_t num_paths = 0, num_name_bytes = 0;
    double prob_precision = 0;
    // the path side: one device block (cluster_path_off, name_off, rank keys, effective lengths, lengths, ids, flags) and the names
    DeviceBuffer<unsigned char> side;
    DeviceBuffer<char> name_bytes;
    size_t at_cluster_path_off = 0, at_name_off = 0, at_lists = 0, at_index = 0, at_eff = 0, at_length = 0, at_id = 0, at_rank = 0;
    void * pinned = nullptr;  // the host copy of both (rpvg_hip_parsed_dump_view)
    ~rpvg_hip_parsed_dump() {
        if (pinned) pinnedFree(pinned);
    }
    template <typename T>
    T * piece(const size_t at) const { return reinterpret_cast<T *>(side.ptr + at); }
};

namespace {

enum Word { kWordBad = 0, kWordNameBytes = 1, kWordExact = 2, kWordLines = 3, kWordTotals = 4, kNumWords = 9 };  // five totals: K, P, R, G, M

__global__ __launch_bounds__(kBlock) void rawFlagsKernel(const char * __restrict__ text, const uint32_t n, uint32_t * line, uint32_t * field, uint32_t * colon, uint32_t * comma) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < n) pp::rawFlags(text, static_cast<uint32_t>(i), line, field, colon, comma);
}

__global__ __launch_bounds__(kBlock) void countFlagsKernel(const pp::Scanned x, uint32_t * markers, uint32_t * paths, uint32_t * rows, uint32_t * groups, uint32_t * indices) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < x.n) pp::countFlags(x, static_cast<uint32_t>(i), markers, paths, rows, groups, indices);
    if (i == x.n) markers[i] = paths[i] = rows[i] = groups[i] = indices[i] = 0;
}

// the last entries of the five sums, beside the offender word: one fetch brings them
__global__ __launch_bounds__(64) void totalsKernel(const pp::Counted c, const uint32_t n, word64 * words) {
    if (threadIdx.x == 0) {
        words[kWordTotals + 0] = c.markers[n];
        words[kWordTotals + 1] = c.paths[n];
        words[kWordTotals + 2] = c.rows[n];
        words[kWordTotals + 3] = c.groups[n];
        words[kWordTotals + 4] = c.indices[n];
    }
}

__global__ __launch_bounds__(kBlock) void markerKernel(const pp::Scanned x, const pp::Counted c, const pp::Parsed o) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < x.n) pp::markerByte(x, c, o, static_cast<uint32_t>(i));
}

struct DeviceSink {
    word64 * words;
    __device__ void report(const uint32_t line_start, const int why) { reportOffender(&words[kWordBad], line_start, why); }
    __device__ void nameBytes(const uint32_t n) {
        if (n) atomicAdd(&words[kWordNameBytes], static_cast<word64>(n));
    }
    __device__ void exactToken() { atomicAdd(&words[kWordExact], static_cast<word64>(1)); }
};

__global__ __launch_bounds__(kBlock) void fillKernel(const pp::Scanned x, const pp::Counted c, const pp::Parsed o, word64 * words) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    DeviceSink sink = {words};
    if (i < x.n) pp::fillByte(x, c, o, static_cast<uint32_t>(i), sink);
}

// the '\n' in front of byte `end`: the 1-based number of the line that starts there, less one (a refused text only)
__global__ __launch_bounds__(kBlock) void linesBeforeKernel(const char * __restrict__ text, const uint32_t end, word64 * words) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    const word64 here = __popcll(__ballot(i < end && text[i] == '\n'));
    if ((threadIdx.x & 63) == 0 && here) atomicAdd(&words[kWordLines], here);
}

__global__ __launch_bounds__(kBlock) void orderKernel(const pp::Groups q) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (g == 0) q.grp_idx_off[q.G] = q.M;
    if (g < q.G) pp::orderGroup(q, g, [&](const uint64_t r) { atomicOr(&q.row_unsorted[r], 1u); });
}

__global__ __launch_bounds__(kBlock) void sortRowsKernel(const pp::Groups q, const uint32_t * __restrict__ row_line, word64 * words) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (r < q.R) pp::sortRow(q, r, [&](const uint64_t row) { reportOffender(&words[kWordBad], row_line[row], pp::kWhyUnsortedRow); });
}

__global__ __launch_bounds__(kBlock) void placeKernel(const pp::Groups q, double * __restrict__ grp_prob, uint32_t * __restrict__ path_idx) {
    const uint64_t j = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    pp::placeEntry(q, j, grp_prob, path_idx);
}

__global__ __launch_bounds__(kBlock) void namesKernel(const char * __restrict__ text, const uint64_t * __restrict__ name_off, const uint32_t * __restrict__ name_src, const uint64_t P,
                                                      const uint64_t num_name_bytes, char * __restrict__ name_bytes) {
    const uint64_t b = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (b < num_name_bytes) name_bytes[b] = pp::nameByte(text, name_off, name_src, P, b);
}

int parseText(rpvg_hip_ctx * ctx, const char * who, const Source<char> & bytes, const uint64_t num_bytes, const double prob_precision, rpvg_hip_parsed_dump ** dump_out) {
    *dump_out = nullptr;
    if (const char * wrong = rpvg_rows_text::probPrecisionBad(prob_precision)) {
        setError("%s: %s (%g)", who, wrong, prob_precision);
        return RPVG_HIP_ERR_INVALID;
    }
    RPVG_REQUIRE(num_bytes <= pp::kMaxTextBytes, "%s: a text of %llu bytes; the limit is %llu (fewer than 2^31 - 1)", who, static_cast<unsigned long long>(num_bytes),
                 static_cast<unsigned long long>(pp::kMaxTextBytes));
    RPVG_REQUIRE(num_bytes == 0 || bytes.from, "%s: NULL text of %llu bytes", who, static_cast<unsigned long long>(num_bytes));
    std::unique_ptr<rpvg_hip_parsed_dump> dump(new (std::nothrow) rpvg_hip_parsed_dump());
    if (dump) dump->rows.reset(new (std::nothrow) rpvg_hip_read_rows());
    if (!dump || !dump->rows) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    dump->ctx = ctx;
    dump->prob_precision = prob_precision;
    rpvg_hip_read_rows * rows = dump->rows.get();
    rows->h_cluster_row_off.assign(1, 0);
    rows->h_cluster_path_off.assign(1, 0);
    const uint32_t n = static_cast<uint32_t>(num_bytes);

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // ---- flags and scans ----
    UploadPack inputs;
    DeviceBuffer<char> text;
    DeviceBuffer<uint64_t> pow10;
    DeviceBuffer<word64> words;
    const word64 initial[kNumWords] = {kNoBad, 0, 0, 0, 0, 0, 0, 0, 0};
    takeInput(inputs, text, bytes, n);
    inputs.add(pow10, pow10Table(), rpvg_number_text::kPow10Words);
    inputs.add(words, initial, kNumWords);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    DeviceBuffer<uint32_t> scans[9];
    for (auto & scan : scans) RPVG_HIP_CHECK(scan.alloc(static_cast<size_t>(n) + 1));
    SpanScope span(ctx, FAM_BUILD);
    word64 h_words[kNumWords] = {kNoBad, 0, 0, 0, 0, 0, 0, 0, 0};
    const pp::Scanned x = {text.ptr, n, scans[0].ptr, scans[1].ptr, scans[2].ptr, scans[3].ptr};
    const pp::Counted c = {scans[4].ptr, scans[5].ptr, scans[6].ptr, scans[7].ptr, scans[8].ptr};
    if (n) {
        rawFlagsKernel<<<gridFor(n), dim3(kBlock), 0, st>>>(text.ptr, n, scans[0].ptr, scans[1].ptr, scans[2].ptr, scans[3].ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        for (int a = 0; a < 4; ++a) {
            if (const int rc = inclusiveScan(st, scans[a].ptr, scans[a].ptr, MaxU32(), n)) return rc;
        }
        countFlagsKernel<<<gridFor(static_cast<uint64_t>(n) + 1), dim3(kBlock), 0, st>>>(x, scans[4].ptr, scans[5].ptr, scans[6].ptr, scans[7].ptr, scans[8].ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        for (int a = 4; a < 9; ++a) {
            if (const int rc = exclusiveSum(st, scans[a].ptr, scans[a].ptr, static_cast<uint64_t>(n) + 1)) return rc;
        }
        totalsKernel<<<dim3(1), dim3(64), 0, st>>>(c, n, words.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 3 + 9;
        if (const int rc = fetchDescribedWords(st, words.ptr, h_words, kNumWords)) return rc;  // the first wait: the totals
    }
    const uint32_t K = static_cast<uint32_t>(h_words[kWordTotals]);
    const uint64_t P = h_words[kWordTotals + 1], R = h_words[kWordTotals + 2], G = h_words[kWordTotals + 3], M = h_words[kWordTotals + 4];

    // ---- the arrays at their exact sizes ----
    size_t side_bytes = 0;
    const auto take = [&](const size_t bytes_wanted) {
        const size_t at = side_bytes;
        side_bytes += UploadPack::aligned(bytes_wanted);
        return at;
    };
    dump->at_cluster_path_off = take((static_cast<size_t>(K) + 1) * sizeof(uint64_t));
    dump->at_name_off = take((static_cast<size_t>(P) + 1) * sizeof(uint64_t));
    dump->at_lists = take(static_cast<size_t>(K) * sizeof(uint64_t));
    dump->at_index = take(static_cast<size_t>(K) * sizeof(uint64_t));
    dump->at_eff = take(static_cast<size_t>(P) * sizeof(double));
    dump->at_length = take(static_cast<size_t>(P) * sizeof(uint32_t));
    dump->at_id = take(static_cast<size_t>(K) * sizeof(uint32_t));
    dump->at_rank = take(static_cast<size_t>(K));
    RPVG_HIP_CHECK(dump->side.alloc(side_bytes));
    RPVG_HIP_CHECK(zeroAsync(dump->side.ptr, side_bytes, st));  // (the padding between the pieces is downloaded with them)
    dump->num_clusters = K;
    dump->num_paths = P;
    rows->num_clusters = K;
    rows->num_rows = R;
    rows->num_groups = G;
    rows->num_members = M;
    RPVG_HIP_CHECK(rows->cluster_row_off.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(rows->row_grp_off.alloc(static_cast<size_t>(R) + 1));
    RPVG_HIP_CHECK(rows->grp_idx_off.alloc(static_cast<size_t>(G) + 1));
    RPVG_HIP_CHECK(rows->row_count.alloc(R));
    RPVG_HIP_CHECK(rows->row_noise.alloc(R));
    RPVG_HIP_CHECK(rows->grp_prob.alloc(G));
    RPVG_HIP_CHECK(rows->path_idx.alloc(M));
    DeviceBuffer<uint32_t> name_src, text_idx, row_unsorted, row_line;
    DeviceBuffer<double> text_prob;
    DeviceBuffer<uint64_t> text_idx_off, source;
    RPVG_HIP_CHECK(name_src.alloc(P));
    RPVG_HIP_CHECK(text_idx.alloc(M));
    RPVG_HIP_CHECK(text_prob.alloc(G));
    RPVG_HIP_CHECK(text_idx_off.alloc(static_cast<size_t>(G) + 1));
    RPVG_HIP_CHECK(source.alloc(G));
    RPVG_HIP_CHECK(row_line.alloc(R));
    RPVG_HIP_CHECK(row_unsorted.alloc(R ? ((R + 1) & ~uint64_t(1)) : 0));
    if (R) RPVG_HIP_CHECK(zeroAsync(row_unsorted.ptr, ((R + 1) & ~uint64_t(1)) * sizeof(uint32_t), st));
    if (n == 0) {  // K = 0: no kernel has anything to do, and the offsets are the host's single zeros
        RPVG_HIP_CHECK(zeroAsync(rows->cluster_row_off.ptr, sizeof(uint64_t), st));
        RPVG_HIP_CHECK(zeroAsync(rows->row_grp_off.ptr, sizeof(uint64_t), st));
        RPVG_HIP_CHECK(zeroAsync(rows->grp_idx_off.ptr, sizeof(uint64_t), st));
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        span.end();
        ctx->parse_stats.calls_completed += 1;
        *dump_out = dump.release();
        return RPVG_HIP_OK;
    }

    pp::Parsed o = {};
    o.K = K;
    o.P = P;
    o.R = R;
    o.G = G;
    o.M = M;
    o.cluster_row_off = rows->cluster_row_off.ptr;
    o.cluster_path_off = dump->piece<uint64_t>(dump->at_cluster_path_off);
    o.has_rank_key = dump->piece<uint8_t>(dump->at_rank);
    o.num_align_lists = dump->piece<uint64_t>(dump->at_lists);
    o.cluster_index = dump->piece<uint64_t>(dump->at_index);
    o.cluster_id = dump->piece<uint32_t>(dump->at_id);
    o.name_len = dump->piece<uint64_t>(dump->at_name_off);
    o.name_src = name_src.ptr;
    o.path_length = dump->piece<uint32_t>(dump->at_length);
    o.path_effective_length = dump->piece<double>(dump->at_eff);
    o.row_count = rows->row_count.ptr;
    o.row_noise = rows->row_noise.ptr;
    o.row_grp_off = rows->row_grp_off.ptr;
    o.row_line = row_line.ptr;
    o.text_prob = text_prob.ptr;
    o.text_idx_off = text_idx_off.ptr;
    o.text_idx = text_idx.ptr;
    o.pow10 = pow10.ptr;

    // ---- fill ----
    markerKernel<<<gridFor(n), dim3(kBlock), 0, st>>>(x, c, o);
    fillKernel<<<gridFor(n), dim3(kBlock), 0, st>>>(x, c, o, words.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 2;
    if (const int rc = fetchDescribedWords(st, words.ptr, h_words, kNumWords)) return rc;  // the second wait: offender, name bytes
    ctx->parse_stats.exact_tokens += h_words[kWordExact];
    const auto refused = [&]() -> int {  // words the message of the offender in h_words with its 1-based line
        const Offender offender = offenderOf(h_words[kWordBad], pp::kWhyLast);
        linesBeforeKernel<<<gridFor(std::max<uint64_t>(offender.index, 1)), dim3(kBlock), 0, st>>>(text.ptr, static_cast<uint32_t>(offender.index), words.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = fetchDescribedWords(st, words.ptr, h_words, kNumWords)) return rc;
        span.end();
        setError("%s: line %llu: %s", who, static_cast<unsigned long long>(h_words[kWordLines] + 1), pp::reasonOf(offender.why));
        return RPVG_HIP_ERR_INVALID;
    };
    if (h_words[kWordBad] != kNoBad) return refused();
    const uint64_t num_name_bytes = h_words[kWordNameBytes];
    dump->num_name_bytes = num_name_bytes;
    RPVG_HIP_CHECK(dump->name_bytes.alloc(num_name_bytes));

    // ---- the order of the groups, and the names ----
    pp::Groups q = {R, G, M, rows->row_grp_off.ptr, text_prob.ptr, text_idx_off.ptr, text_idx.ptr, row_unsorted.ptr, source.ptr, rows->grp_idx_off.ptr};
    orderKernel<<<gridFor(std::max<uint64_t>(G, 1)), dim3(kBlock), 0, st>>>(q);
    if (R) sortRowsKernel<<<gridFor(R), dim3(kBlock), 0, st>>>(q, row_line.ptr, words.ptr);
    if (G) placeKernel<<<gridFor(std::max<uint64_t>(G, M)), dim3(kBlock), 0, st>>>(q, rows->grp_prob.ptr, rows->path_idx.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 3;
    if (const int rc = exclusiveSum(st, o.name_len, o.name_len, P + 1)) return rc;
    if (num_name_bytes) {
        namesKernel<<<gridFor(num_name_bytes), dim3(kBlock), 0, st>>>(text.ptr, o.name_len, name_src.ptr, P, num_name_bytes, dump->name_bytes.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
    }
    rows->h_cluster_row_off.assign(static_cast<size_t>(K) + 1, 0);
    rows->h_cluster_path_off.assign(static_cast<size_t>(K) + 1, 0);
    RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_cluster_row_off.data(), rows->cluster_row_off.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_cluster_path_off.data(), o.cluster_path_off, (static_cast<size_t>(K) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (const int rc = fetchDescribedWords(st, words.ptr, h_words, kNumWords)) return rc;  // the last wait; the scans and the text's order go back to the pool
    if (h_words[kWordBad] != kNoBad) return refused();  // (an unsorted row too long to sort: only found behind a text without another offence)
    span.end();
    ctx->parse_stats.calls_completed += 1;
    *dump_out = dump.release();
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" {

int rpvg_hip_text_rows(rpvg_hip_ctx * ctx, const char * bytes, uint64_t n, int32_t on_device, double prob_precision, rpvg_hip_parsed_dump ** dump_out) {
    const char * const who = "rpvg_hip_text_rows";
    RPVG_REQUIRE(ctx && dump_out, "%s: NULL argument", who);
    return parseText(ctx, who, Source<char>{bytes, on_device != 0}, n, prob_precision, dump_out);
}

int rpvg_hip_table_text_rows(rpvg_hip_table_text * text, double prob_precision, rpvg_hip_parsed_dump ** dump_out) {
    const char * const who = "rpvg_hip_table_text_rows";
    RPVG_REQUIRE(text && text->ctx && dump_out, "%s: NULL argument", who);
    return parseText(text->ctx, who, Source<char>{text->num_bytes ? text->text() : nullptr, true}, text->num_bytes, prob_precision, dump_out);
}

rpvg_hip_read_rows * rpvg_hip_parsed_dump_rows(rpvg_hip_parsed_dump * dump) { return dump ? dump->rows.get() : nullptr; }

int rpvg_hip_parsed_dump_view(rpvg_hip_parsed_dump * dump, rpvg_parsed_dump_view * view_out) {
    const char * const who = "rpvg_hip_parsed_dump_view";
    RPVG_REQUIRE(dump && view_out, "%s: NULL argument", who);
    const size_t side_bytes = dump->side.count, names = static_cast<size_t>(dump->num_name_bytes);
    if (!dump->pinned) {
        rpvg_hip_ctx * ctx = dump->ctx;
        std::lock_guard<std::mutex> lock(ctx->mutex);
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        void * pinned = nullptr;
        if (pinnedAlloc(&pinned, side_bytes + names + 1) != hipSuccess) {
            setError("%s: no page-locked memory for %llu bytes", who, static_cast<unsigned long long>(side_bytes + names));
            return RPVG_HIP_ERR_ALLOC;
        }
        hipError_t e = hipMemcpyAsync(pinned, dump->side.ptr, side_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && names) e = hipMemcpyAsync(static_cast<char *>(pinned) + side_bytes, dump->name_bytes.ptr, names, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) pinnedFree(pinned);
        RPVG_HIP_CHECK(e);
        dump->pinned = pinned;
    }
    const unsigned char * host = static_cast<const unsigned char *>(dump->pinned);
    std::memset(view_out, 0, sizeof(*view_out));
    view_out->num_clusters = dump->num_clusters;
    view_out->num_paths = dump->num_paths;
    view_out->num_name_bytes = dump->num_name_bytes;
    view_out->cluster_path_off = reinterpret_cast<const uint64_t *>(host + dump->at_cluster_path_off);
    view_out->name_off = reinterpret_cast<const uint64_t *>(host + dump->at_name_off);
    view_out->name_bytes = reinterpret_cast<const char *>(host + side_bytes);
    view_out->path_length = reinterpret_cast<const uint32_t *>(host + dump->at_length);
    view_out->path_effective_length = reinterpret_cast<const double *>(host + dump->at_eff);
    view_out->has_rank_key = reinterpret_cast<const uint8_t *>(host + dump->at_rank);
    view_out->num_align_lists = reinterpret_cast<const uint64_t *>(host + dump->at_lists);
    view_out->cluster_index = reinterpret_cast<const uint64_t *>(host + dump->at_index);
    return RPVG_HIP_OK;
}

int rpvg_hip_parsed_dump_labels(rpvg_hip_parsed_dump * dump, rpvg_table_labels * labels_out) {
    RPVG_REQUIRE(dump && labels_out, "rpvg_hip_parsed_dump_labels: NULL argument");
    std::memset(labels_out, 0, sizeof(*labels_out));
    labels_out->num_clusters = dump->num_clusters;
    labels_out->num_paths = dump->num_paths;
    labels_out->num_name_bytes = dump->num_name_bytes;
    labels_out->name_off = dump->piece<uint64_t>(dump->at_name_off);
    labels_out->name_bytes = dump->name_bytes.ptr;
    labels_out->path_length = dump->piece<uint32_t>(dump->at_length);
    labels_out->cluster_id = dump->piece<uint32_t>(dump->at_id);
    labels_out->on_device = 1;
    return RPVG_HIP_OK;
}

int rpvg_hip_parse_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_parse_stats * stats_out) {
    RPVG_REQUIRE(ctx && stats_out, "rpvg_hip_parse_stats_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    *stats_out = ctx->parse_stats;
    return RPVG_HIP_OK;
}

void rpvg_hip_parsed_dump_free(rpvg_hip_parsed_dump * dump) {
    if (!dump) return;
    waitAndDelete(dump->ctx);
    delete dump;
}

}  // extern "C"
