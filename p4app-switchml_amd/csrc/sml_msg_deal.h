// sml_msg_deal.h — how a long RDMA message is dealt to the waves of one
// workgroup, shared by the plane kernels (sml_messages.hip) and the worker's
// completion loop for long messages (sml_msg_worker.hip).  A message of M
// elements is cut into ceil(M / 256) slices of one wave-wide 16-byte access
// and occupies wpm = ceil(M / 1024) waves; slice s goes to wave s % wpm as
// that wave's slice s / wpm, so a wave keeps at most 4 slices and the waves'
// accesses of one round are consecutive KiB of the message.  sml_messages.hip
// records why wpm is a launch parameter and not rounded up to a power of two.
#ifndef SML_MSG_DEAL_H_
#define SML_MSG_DEAL_H_

#include "sml_device.h"

namespace sml {

constexpr int kMsgU = 4;                       // slices a wave keeps of its message
constexpr int kMsgMaxWaves = 16;               // waves of the largest message = of the largest workgroup

// Waves a message of M elements occupies.
inline uint32_t msg_waves(uint32_t M) { return (M + kTileElems - 1) / kTileElems; }

// Offset inside its message of the vector this lane holds as slice u of wave
// `part` of the message.
__device__ __forceinline__ uint32_t msg_offset(uint32_t wpm, int u, uint32_t part, int lane) {
    return ((uint32_t)u * wpm + part) * 256u + (uint32_t)lane * 4u;
}

}  // namespace sml

#endif  // SML_MSG_DEAL_H_
