/*
 * Stand-alone driver of the reference's dummy-backend Context, compiled from
 * the reference checkout into oracle/_ref/ref_allreduce (see the Makefile).
 *
 * TEST INFRASTRUCTURE ONLY: the bit-level pin of the oracle's packet loop
 * (oracle/sml_oracle.c: orc_dummy_allreduce) and slice geometry.  This file is
 * the project's own text; it names reference headers and calls the Context's
 * public methods, nothing more.
 *
 *   ref_allreduce W T P MOP PROCESS TYPE INPLACE IN OUT OFFSET:NUMEL [...]
 *
 *   W, T, P, MOP   num_workers, num_worker_threads, packet_numel,
 *                  max_outstanding_packets
 *   PROCESS        1: the dummy backend multiplies every packet by W
 *   TYPE           f32 | i32
 *   INPLACE        1: every job reduces its part of the buffer in place;
 *                  0: into the same part of a second, zero-filled buffer
 *   IN, OUT        raw 32-bit words: the whole input buffer is read from IN,
 *                  the whole result buffer is written to OUT
 *   OFFSET:NUMEL   one all-reduce job over elements [OFFSET, OFFSET+NUMEL) of
 *                  the buffer; the jobs are submitted in the order given and
 *                  waited for together.
 *
 * The Context is a singleton that starts once, so every run is a fresh
 * process.  The four Config members below live in the reference's config.cc,
 * which needs boost; no file is parsed here, so they are defined as the
 * plain operations the driver needs.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "config.h"
#include "context.h"
#include "job.h"

namespace google {
namespace glog_internal_namespace_ {
bool IsGoogleLoggingInitialized() { return true; }
}  // namespace glog_internal_namespace_
}  // namespace google
std::string FLAGS_vmodule;

namespace switchml {
void Config::operator=(Config const& other) {
    this->general_ = other.general_;
    this->backend_ = other.backend_;
}
bool Config::LoadFromFile(std::string) { return false; }
void Config::Validate() {}
void Config::PrintConfig() {}
}  // namespace switchml

static int usage() {
    std::fprintf(stderr, "usage: ref_allreduce W T P MOP PROCESS f32|i32 INPLACE IN OUT OFFSET:NUMEL [...]\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 11) return usage();
    switchml::Config config;
    config.general_.rank = 0;
    config.general_.num_workers = static_cast<uint16_t>(std::strtoul(argv[1], nullptr, 10));
    config.general_.num_worker_threads = static_cast<uint16_t>(std::strtoul(argv[2], nullptr, 10));
    config.general_.packet_numel = std::strtoull(argv[3], nullptr, 10);
    config.general_.max_outstanding_packets = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10));
    config.general_.backend = "dummy";
    config.general_.scheduler = "fifo";
    config.general_.prepostprocessor = "cpu_exponent_quantizer";
    config.general_.instant_job_completion = false;
    config.general_.controller_ip_str = "127.0.0.1";
    config.general_.controller_port = 50099;
    config.backend_.dummy.bandwidth = 0;
    config.backend_.dummy.process_packets = std::atoi(argv[5]) != 0;
    if (config.general_.num_worker_threads == 0 ||
        config.general_.max_outstanding_packets / config.general_.num_worker_threads == 0 ||
        config.general_.packet_numel == 0)
        return usage();

    switchml::DataType type;
    if (!std::strcmp(argv[6], "f32")) type = switchml::FLOAT32;
    else if (!std::strcmp(argv[6], "i32")) type = switchml::INT32;
    else return usage();
    const bool inplace = std::atoi(argv[7]) != 0;

    std::FILE* f = std::fopen(argv[8], "rb");
    if (!f) { std::perror(argv[8]); return 1; }
    std::fseek(f, 0, SEEK_END);
    const size_t total = static_cast<size_t>(std::ftell(f)) / 4;
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> in(total + 1), out(total + 1, 0u);
    if (std::fread(in.data(), 4, total, f) != total) { std::fclose(f); return 1; }
    std::fclose(f);

    struct JobSpec { uint64_t offset, numel; };
    std::vector<JobSpec> specs;
    for (int a = 10; a < argc; a++) {
        char* colon = nullptr;
        JobSpec s;
        s.offset = std::strtoull(argv[a], &colon, 10);
        if (!colon || *colon != ':') return usage();
        s.numel = std::strtoull(colon + 1, nullptr, 10);
        if (s.offset + s.numel > total) { std::fprintf(stderr, "job %s exceeds the buffer\n", argv[a]); return 2; }
        specs.push_back(s);
    }

    switchml::Context& ctx = switchml::Context::GetInstance();
    if (!ctx.Start(&config)) return 1;
    std::vector<std::shared_ptr<switchml::Job>> jobs;
    for (const JobSpec& s : specs) {
        uint32_t* src = in.data() + s.offset;
        uint32_t* dst = (inplace ? in.data() : out.data()) + s.offset;
        jobs.push_back(ctx.AllReduceAsync(src, dst, s.numel, type, switchml::AllReduceOperation::SUM));
    }
    ctx.WaitForAllJobs();
    int rc = 0;
    for (auto& j : jobs)
        if (j->GetJobStatus() != switchml::JobStatus::FINISHED) rc = 3;

    f = std::fopen(argv[9], "wb");
    if (!f) { std::perror(argv[9]); return 1; }
    const uint32_t* res = inplace ? in.data() : out.data();
    if (std::fwrite(res, 4, total, f) != total) rc = 1;
    std::fclose(f);
    ctx.Stop();
    return rc;
}
