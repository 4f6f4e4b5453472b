/*
 * C ABI over the reference's CpuExponentQuantizerPPP, compiled from the
 * reference checkout into oracle/_ref/libsml_ref_ppp*.so (see the Makefile).
 *
 * TEST INFRASTRUCTURE ONLY: the bit-level pin of oracle/sml_oracle.c.  This
 * file is the project's own text; it names reference headers and calls the
 * class's public methods, nothing more.  Python drives the call order
 * (oracle/oracle.py: RefPPP); the *_range calls only loop over consecutive
 * ltu ids so that a plane does not cost one foreign call per packet.
 */
#include <cstdint>
#include <string>

#include "config.h"
#include "job.h"
#include "cpu_exponent_quantizer_ppp.h"

/* What the reference expects glog to define (glog_fix.h). */
namespace google {
namespace glog_internal_namespace_ {
bool IsGoogleLoggingInitialized() { return true; }
}  // namespace glog_internal_namespace_
}  // namespace google
std::string FLAGS_vmodule;

namespace {
struct Handle {
    switchml::Config config;
    switchml::JobSlice slice;
    switchml::CpuExponentQuantizerPPP* ppp;
};
}  // namespace

extern "C" {

void* refppp_create(uint16_t num_workers, uint64_t ltu_bytes, uint64_t batch_num_ltus) {
    Handle* h = new Handle();
    h->config.general_.num_workers = num_workers;
    h->config.general_.prepostprocessor = "cpu_exponent_quantizer";
    h->ppp = new switchml::CpuExponentQuantizerPPP(h->config, 0, ltu_bytes, batch_num_ltus);
    return h;
}

/* data_type: 0 = FLOAT32, 1 = INT32.  Returns the number of main ltus. */
uint64_t refppp_setup(void* handle, void* in, void* out, uint64_t numel, int data_type) {
    Handle* h = static_cast<Handle*>(handle);
    h->ppp->CleanupJobSlice();
    h->slice.job = nullptr;
    h->slice.slice.in_ptr = in;
    h->slice.slice.out_ptr = out;
    h->slice.slice.numel = numel;
    h->slice.slice.data_type = data_type == 0 ? switchml::FLOAT32 : switchml::INT32;
    return h->ppp->SetupJobSlice(&h->slice);
}

int refppp_needs_extra_batch(void* handle) {
    return static_cast<Handle*>(handle)->ppp->NeedsExtraBatch() ? 1 : 0;
}

void refppp_pre(void* handle, uint64_t ltu_id, void* entries, void* exponent) {
    static_cast<Handle*>(handle)->ppp->PreprocessSingle(ltu_id, entries, exponent);
}

void refppp_post(void* handle, uint64_t ltu_id, void* entries, void* exponent) {
    static_cast<Handle*>(handle)->ppp->PostprocessSingle(ltu_id, entries, exponent);
}

/* ltu ids first .. first+count-1; packet k of the range has its entries at
 * entries + k*entries_stride and its exponent slot at exponents + k*exp_stride
 * (strides in bytes; 0 points every packet at the same place). */
void refppp_pre_range(void* handle, uint64_t first, uint64_t count, void* entries, uint64_t entries_stride,
                      void* exponents, uint64_t exp_stride) {
    Handle* h = static_cast<Handle*>(handle);
    for (uint64_t k = 0; k < count; k++)
        h->ppp->PreprocessSingle(first + k, static_cast<char*>(entries) + k * entries_stride,
                                 static_cast<char*>(exponents) + k * exp_stride);
}

void refppp_post_range(void* handle, uint64_t first, uint64_t count, void* entries, uint64_t entries_stride,
                       void* exponents, uint64_t exp_stride) {
    Handle* h = static_cast<Handle*>(handle);
    for (uint64_t k = 0; k < count; k++)
        h->ppp->PostprocessSingle(first + k, static_cast<char*>(entries) + k * entries_stride,
                                  static_cast<char*>(exponents) + k * exp_stride);
}

void refppp_destroy(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    delete h->ppp;
    delete h;
}

}  // extern "C"
