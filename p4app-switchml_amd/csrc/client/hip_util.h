// hip_util.h — what the client's HIP-facing files share: the error checks and
// the one "where does this pointer live" query.  Internal to csrc/client.
#ifndef SWITCHML_AMD_HIP_UTIL_H_
#define SWITCHML_AMD_HIP_UTIL_H_

#include <hip/hip_runtime_api.h>

#include <string>

#include "common.h"
#include "switchml_hip.h"

namespace switchml {

// Throw SwitchMLFatal("<prefix><what>: <error>") unless the call succeeded.
inline void hip_ok(hipError_t e, const char* what, const char* prefix = "") {
    if (e != hipSuccess) throw SwitchMLFatal(std::string(prefix) + what + ": " + hipGetErrorString(e));
}

inline void sml_ok(int s, const char* what, const char* prefix = "") {
    if (s != SML_OK)
        throw SwitchMLFatal(std::string(prefix) + what + ": " + sml_status_string((sml_status_t)s) + " " +
                            sml_last_error());
}

// Where a buffer lives.  Device (and managed) memory and pinned (page-locked,
// device-mapped) host memory are read and written by the kernels directly;
// pageable host memory, or a pointer HIP does not know, is staged.
struct PointerInfo {
    void* dev = nullptr;   // the address a kernel can use, null for pageable memory
    bool device = false;   // device or managed memory: the CPU does not touch it
    bool host() const { return !device; }             // the CPU may touch it right after a call returns
    bool host_mapped() const { return dev && !device; }
};

inline PointerInfo QueryPointer(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // not an error of the caller's: clear the sticky status
        return {};
    }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) return {const_cast<void*>(p), true};
    if (a.type == hipMemoryTypeHost && a.devicePointer) return {a.devicePointer, false};
    return {};
}

}  // namespace switchml

#endif  // SWITCHML_AMD_HIP_UTIL_H_
