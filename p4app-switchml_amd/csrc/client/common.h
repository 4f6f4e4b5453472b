// common.h — value types of the SwitchML client API, MI355X build.
//
// Mirrors the names and meaning of client_lib/src/common.h:35-116 and
// job.h:36-70 (reference paths relative to /root/reference/dev_root/) so code
// written against the reference compiles unchanged against this header.
// Tensor pointers may be HOST or DEVICE memory: the loopback backend detects
// which (QueryPointer, hip_util.h) and stages host tensors through HBM.
#ifndef SWITCHML_AMD_COMMON_H_
#define SWITCHML_AMD_COMMON_H_

#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <thread>

namespace switchml {

typedef uint64_t JobId;
typedef int16_t WorkerTid;
typedef uint64_t Numel;
typedef std::chrono::steady_clock clock;

// common.h:51-55; FLOAT16 (IEEE binary16) and BFLOAT16 are this build's: the
// kernels widen them to fp32 on the way in and narrow on the way out, so they
// travel as FLOAT32 does (int32 words, one exponent per packet).
enum DataType { FLOAT32, INT32, FLOAT16, BFLOAT16 };

inline bool IsHalfType(DataType type) { return type == FLOAT16 || type == BFLOAT16; }
// Float types are quantized: an exponent per packet, hence the extra batch.
inline bool IsFloatType(DataType type) { return type == FLOAT32 || IsHalfType(type); }
inline const char* DataTypeName(DataType type) {
    switch (type) {
        case FLOAT32: return "FLOAT32";
        case INT32: return "INT32";
        case FLOAT16: return "FLOAT16";
        case BFLOAT16: return "BFLOAT16";
    }
    return "?";
}

// job.h:36-39 / 44-46
enum JobType { ALLREDUCE, BROADCAST };
enum AllReduceOperation { SUM };
union ExtraJobInfo {
    AllReduceOperation allreduce_operation;
    int32_t broadcast_root_rank;
};

// The reference aborts with LOG(FATAL) on these conditions; this build throws
// (the C-ABI wrappers convert it to an error code).
class SwitchMLFatal : public std::runtime_error {
  public:
    explicit SwitchMLFatal(const std::string& what) : std::runtime_error(what) {}
};

// common.h:62-70
inline uint16_t DataTypeSize(DataType type) {
    if (type == FLOAT32 || type == INT32) return 4;
    if (type == FLOAT16 || type == BFLOAT16) return 2;
    throw SwitchMLFatal("'" + std::to_string((int)type) + "' is not a valid tensor data type");
}

// common.h:75-116: a borrowed view of the caller's input/output memory.
struct Tensor {
    void* in_ptr;
    void* out_ptr;
    Numel numel;
    DataType data_type;

    // Advance both pointers by `numel` ELEMENTS of data_type; numel untouched.
    void OffsetPtrs(Numel n) {
        const Numel bytes = n * DataTypeSize(data_type);
        in_ptr = static_cast<char*>(in_ptr) + bytes;
        out_ptr = static_cast<char*>(out_ptr) + bytes;
    }
};

// Bytes a slice takes on the wire: every element travels as one 32-bit word,
// a 16-bit element too (a packet is ltu_size / 4 words whatever the type), so
// the packet count is ceil(numel / P) and never halves for 2-byte elements.
inline Numel WireBytes(const Tensor& t) {
    (void)DataTypeSize(t.data_type);   // throws on an invalid type
    return t.numel * 4;
}

// How long a waiter polls before it sleeps (job completion, a worker's
// stream, an idle worker waiting for the next job), in microseconds.
// SWITCHML_SPIN_US overrides the default; 0 = always sleep at once.
int SpinMicros();

// The poll before every sleep: call done() until it holds or SpinMicros() has
// passed (once at least), yielding the CPU between polls if asked to.  Returns
// whether it held; what a waiter does when it did not (block on the stream or
// event, sleep on a condition variable) is the caller's.
template <class Pred>
bool SpinUntil(Pred done, bool yield_between = false) {
    const auto until = clock::now() + std::chrono::microseconds(SpinMicros());
    do {
        if (done()) return true;
        if (yield_between) std::this_thread::yield();
    } while (clock::now() < until);
    return false;
}

}  // namespace switchml

#endif  // SWITCHML_AMD_COMMON_H_
