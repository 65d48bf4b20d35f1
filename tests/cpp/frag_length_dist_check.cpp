// The host classes of the fragment-length model through their C++ interface — FragmentLengthDist(counts, skew_normal)
// fitted on the GPU and effectivePathLengths (rpvg_amd/host/read_rows.hpp) — against the sequential loop of
// rpvg_amd/csrc/frag_math.hpp on one host thread, which is also the CPU line the device is timed against
// (the reference fits on one thread, src/main.cpp:235).
//
//   frag_length_dist_check <file with one count per line> [paths to time the effective lengths on]
//
// Prints the fits, the timings and "ok".
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "frag_math.hpp"
#include "read_rows.hpp"

namespace {

double seconds(const std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
}

int fail(const char * what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

}  // namespace

int main(int argc, char ** argv) {
    if (argc < 2) {
        std::printf("usage: frag_length_dist_check <counts file> [paths]\n");
        return 0;
    }
    std::vector<uint32_t> counts;
    {
        std::ifstream in(argv[1]);
        uint64_t value;
        while (in >> value) counts.push_back(static_cast<uint32_t>(value));
    }
    if (counts.empty() || counts.front() != 0) return fail("the counts file");
    const size_t timed_paths = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 0;

    const rpvg_frag::GaussLegendre gl = rpvg_frag::makeGaussLegendre();
    auto engine = rpvg_amd::HipEngine::processDefault();

    for (const bool skew_normal : {true, false}) {
        // the sequential line
        rpvg_frag::SequentialSums sums{counts.data(), static_cast<uint32_t>(counts.size())};
        auto start = std::chrono::steady_clock::now();
        const rpvg_frag::FitResult host = rpvg_frag::fitFragmentLengths(sums, static_cast<uint32_t>(counts.size()), skew_normal);
        const double host_s = seconds(start);

        // the class, fitted on the device (the second construction is the warm one)
        rpvg_amd::FragmentLengthDist first(counts, skew_normal, engine);
        start = std::chrono::steady_clock::now();
        const rpvg_amd::FragmentLengthDist dist(counts, skew_normal, engine);
        const double device_s = seconds(start);

        std::printf("%s fit of %zu counts: host loc %.12g scale %.12g shape %.12g (%u iterations, %u evaluations, %.3f ms on one thread); "
                    "device loc %.12g scale %.12g shape %.12g (%u iterations, %u evaluations, %.3f ms with the table of the class)\n",
                    skew_normal ? "skew-normal" : "normal", counts.size(), host.loc, host.scale, host.shape, host.iterations, host.evaluations,
                    host_s * 1e3, dist.loc(), dist.scale(), dist.shape(), dist.fitIterations(), dist.fitEvaluations(), device_s * 1e3);

        if (!dist.isValid() || !host.valid) return fail("an invalid fit");
        if (dist.maxLength() != counts.size()) return fail("maxLength");
        if (std::fabs(dist.loc() - host.loc) >= 1e-3 || std::fabs(dist.scale() - host.scale) >= 1e-3 || std::fabs(dist.shape() - host.shape) >= 1e-3) {
            return fail("device and host fits differ by 1e-3 or more");
        }
        if (first.loc() != dist.loc() || first.scale() != dist.scale() || first.shape() != dist.shape()) return fail("two fits, two results");

        // logProb: the buffer of counts.size() + 1 entries and the formula beyond it are the same function
        for (const uint32_t value : {0u, 1u, static_cast<uint32_t>(counts.size()) - 1, static_cast<uint32_t>(counts.size()),
                                     static_cast<uint32_t>(counts.size()) + 1, 40000u, 65535u}) {
            const double want = rpvg_frag::logProb(value, dist.loc(), dist.scale(), dist.shape());
            if (!(std::fabs(dist.logProb(value) - want) <= 1e-12 * std::fabs(want))) return fail("logProb");
        }
        const std::vector<double> table = dist.logProbTable();
        const std::vector<double> device_table = rpvg_amd::DeviceFragmentLengthTable(engine, dist).download();
        for (size_t v = 0; v < table.size(); ++v) {
            if (!(std::fabs(device_table[v] - table[v]) <= 1e-9 * std::fabs(table[v]))) return fail("the device table");
        }

        // effective lengths: every length below 2048 and a few large ones, where the truncated mean has a denominator
        std::vector<uint32_t> lengths;
        for (uint32_t length = 0; length < 2048; ++length) lengths.push_back(length);
        for (const uint32_t length : {5000u, 100000u, 4000000u, 4294967295u, 1u}) lengths.push_back(length);
        const std::vector<double> effective = rpvg_amd::effectivePathLengths(engine, lengths, dist);
        const rpvg_frag::EffectiveLengthLower lower = rpvg_frag::effectiveLengthLower(dist.loc(), dist.scale(), dist.shape(), gl);
        size_t compared = 0;
        for (size_t i = 0; i < lengths.size(); ++i) {
            const double want = rpvg_frag::effectivePathLength(lengths[i], dist.loc(), dist.scale(), dist.shape(), lower, gl);
            if (lengths[i] == 0) {
                if (effective[i] != 0) return fail("length 0");
                continue;
            }
            if (!std::isfinite(effective[i]) || effective[i] < 1) return fail("an effective length below 1");
            double denominator = 1;
            if (!rpvg_frag::doubleCompare(dist.shape(), 0.0)) {
                rpvg_frag::truncatedSkewNormalMean(dist.loc(), dist.scale(), dist.shape(), lower.bound, lengths[i], gl, &denominator);
            } else {
                denominator = rpvg_frag::upperPhi((lengths[i] - dist.loc()) / dist.scale()) - lower.upper_phi;
            }
            if (denominator < 1e-6) continue;
            ++compared;
            if (!(std::fabs(effective[i] - want) <= 1e-6 * want)) return fail("an effective length");
        }
        if (compared < 500) return fail("too few effective lengths compared");
    }

    if (timed_paths) {
        const rpvg_amd::FragmentLengthDist dist(counts, true, engine);
        std::vector<uint32_t> lengths(timed_paths);
        for (size_t i = 0; i < timed_paths; ++i) lengths[i] = 200 + static_cast<uint32_t>((i * 2654435761ull) % 9800);
        rpvg_amd::effectivePathLengths(engine, lengths, dist);
        auto start = std::chrono::steady_clock::now();
        const std::vector<double> effective = rpvg_amd::effectivePathLengths(engine, lengths, dist);
        const double device_s = seconds(start);
        const rpvg_frag::EffectiveLengthLower lower = rpvg_frag::effectiveLengthLower(dist.loc(), dist.scale(), dist.shape(), gl);
        std::vector<double> host(timed_paths);
        start = std::chrono::steady_clock::now();
        for (size_t i = 0; i < timed_paths; ++i) host[i] = rpvg_frag::effectivePathLength(lengths[i], dist.loc(), dist.scale(), dist.shape(), lower, gl);
        const double host_s = seconds(start);
        double worst = 0;
        for (size_t i = 0; i < timed_paths; ++i) worst = std::fmax(worst, std::fabs(effective[i] - host[i]) / host[i]);
        std::printf("effective lengths of %zu paths: %.3f ms on the device (upload and download included), %.3f ms on one host thread, "
                    "largest relative difference %.3g\n", timed_paths, device_s * 1e3, host_s * 1e3, worst);
        if (!(worst <= 1e-6)) return fail("timed effective lengths");
    }

    std::printf("ok\n");
    return 0;
}
