// sml_packet_phases.h — the phases of one packet (or RDMA message) held by one
// wave, shared by the per-packet bursts (sml_packets.hip) and the RDMA worker's
// completion loop (sml_rdma_worker.hip): how a wave holds P words, how it loads
// and stores them from a packet buffer or a block of the job slice, and the
// three pieces of PreprocessSingle / PostprocessSingle (ppp.cc:69-192, 194-299)
// — the block's exponent, the block packed into wire words, the wire words
// unpacked into the output.  Each rule is written once, here.
#ifndef SML_PACKET_PHASES_H_
#define SML_PACKET_PHASES_H_

#include "sml_device.h"
#include "switchml_hip.h"

namespace sml {

// A packet of P words is held by one wave as U slices of 256 words: lane l
// holds words [j(u), j(u) + 4), j(u) = 256 u + 4 l.  Every phase touches
// words j + t < n only, and n <= P, so the lanes past a packet of fewer than
// 256 words (4 l >= P) drop out of every phase without a test of their own.
template <int P>
struct PacketLanes {
    static constexpr int U = P > 256 ? P / 256 : 1;
    const int lane = threadIdx.x & (kWave - 1);
    __device__ __forceinline__ uint64_t j(int u) const { return (uint64_t)u * 256 + lane * 4; }
};

// A lane's four words [j, j + 4) of the n words of a buffer: one 16-byte access
// where the group is whole (a packet over PCIe then costs one access per 64 B
// line, not four), single words in the group that n cuts.  The load gives 0
// past n; the store writes nothing at or past n.
__device__ __forceinline__ void load_group(const uint32_t* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
    if (j + 4 <= n) {
        const u4a q = *reinterpret_cast<const u4a*>(buf + j);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = j + t < n ? buf[j + t] : 0u;
    }
}

__device__ __forceinline__ void store_group(uint32_t* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
    if (j + 4 <= n) {
        *reinterpret_cast<u4a*>(buf + j) = u4a{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (j + t < n) buf[j + t] = v[t];
    }
}

// What a buffer's elements are to load_group / store_group: the words
// themselves (packet buffers; FLOAT32 and INT32 slices, whose elements are
// their bits), or 16-bit floats held as fp32 bits in registers (FLOAT16 /
// BFLOAT16 slices).  is_float: whether the slice takes the float rules — a
// 16-bit instance has no INT32 branch.
struct SliceWords {
    typedef uint32_t raw;
    static __device__ __forceinline__ bool is_float(const sml_packet_burst& a) { return a.data_type == SML_FLOAT32; }
    static __device__ __forceinline__ void load_group(const raw* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
        sml::load_group(buf, j, n, v);
    }
    static __device__ __forceinline__ void store_group(raw* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
        sml::store_group(buf, j, n, v);
    }
};

// A lane's four elements are one 8-byte access through the 2-byte-aligned
// vector type where the group is whole (a slice starts at any element),
// single elements in the group that n cuts; widened (exact) right after the
// load, narrowed (round to nearest even) right before the store.
template <int H>
struct Slice16 {
    typedef uint16_t raw;
    static __device__ __forceinline__ bool is_float(const sml_packet_burst&) { return true; }
    static __device__ __forceinline__ void load_group(const raw* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
        if (j + 4 <= n) {
            const h4a q = *reinterpret_cast<const h4a*>(buf + j);
            v[0] = __float_as_uint(widen16<H>(q.x)), v[1] = __float_as_uint(widen16<H>(q.y));
            v[2] = __float_as_uint(widen16<H>(q.z)), v[3] = __float_as_uint(widen16<H>(q.w));
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) v[t] = j + t < n ? __float_as_uint(widen16<H>(buf[j + t])) : 0u;
        }
    }
    static __device__ __forceinline__ void store_group(raw* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
        if (j + 4 <= n) {
            *reinterpret_cast<h4a*>(buf + j) =
                h4a{narrow16<H>(__uint_as_float(v[0])), narrow16<H>(__uint_as_float(v[1])),
                    narrow16<H>(__uint_as_float(v[2])), narrow16<H>(__uint_as_float(v[3]))};
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (j + t < n) buf[j + t] = narrow16<H>(__uint_as_float(v[t]));
        }
    }
};

// Elements [0, n) of a buffer <-> w: a packet buffer's words (E = SliceWords),
// or a block of the slice as fp32 bits.
template <class E = SliceWords, int P, int U>
__device__ __forceinline__ void load_words(PacketLanes<P> g, const typename E::raw* buf, uint64_t n,
                                           uint32_t (&w)[U][4]) {
#pragma unroll
    for (int u = 0; u < U; u++) E::load_group(buf, g.j(u), n, w[u]);
}

template <class E = SliceWords, int P, int U>
__device__ __forceinline__ void store_words(PacketLanes<P> g, typename E::raw* buf, uint64_t n,
                                            const uint32_t (&w)[U][4]) {
#pragma unroll
    for (int u = 0; u < U; u++) E::store_group(buf, g.j(u), n, w[u]);
}

__device__ __forceinline__ f4 as_f4(const uint32_t (&v)[4]) {
    return mkf4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// The exponent of the block in x (0 past its real words), the same value in
// every lane: the DPP row reduce, then the four rows through SGPRs.
template <int P, int U>
__device__ __forceinline__ int block_exponent(PacketLanes<P>, const uint32_t (&x)[U][4]) {
    uint32_t m = 0;
#pragma unroll
    for (int u = 0; u < U; u++) m = umax(m, max4(as_f4(x[u])));
    return exponent_of(group_max<256>(m));                  // the wave's max = the packet's
}

// That exponent into byte 0 of the packet's extra-info slot; byte 1 is never
// written (ppp.cc:154).
template <int P, int U>
__device__ __forceinline__ void store_block_exponent(PacketLanes<P> g, const uint32_t (&x)[U][4], void* extra) {
    const int e = block_exponent(g, x);
    if (g.lane == 0) *static_cast<int8_t*>(extra) = (int8_t)e;
}

// The n words of the block in x, big-endian, into w; the other words of w
// keep their value.  FLOAT32: quantized with scale s, VCL=1 rounding (RNE) on
// the 16-aligned body of the block; INT32: as they are.
template <int P, bool RNE, int U>
__device__ __forceinline__ void pack_block(PacketLanes<P> g, bool flt, const uint32_t (&x)[U][4], float s, uint64_t n,
                                           uint32_t (&w)[U][4]) {
    const uint64_t body = n / 16 * 16;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t j = g.j(u);
        const u4 v = flt ? quantize4<RNE>(as_f4(x[u]), s, j, body) : mku4(x[u][0], x[u][1], x[u][2], x[u][3]);
        const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (j + t < n) w[u][t] = bswap(vv[t]);
    }
}

// Words [0, n) of w into the n elements of a block of the output: dequantized
// with scale s (a float type; a 16-bit one narrowed by E's store), or
// byte-swapped (INT32).
template <class E, int P, int U>
__device__ __forceinline__ void unpack_block(PacketLanes<P> g, bool flt, const uint32_t (&w)[U][4], float s, uint64_t n,
                                             typename E::raw* out) {
#pragma unroll
    for (int u = 0; u < U; u++) {
        uint32_t v[4];   // every word of the group converted, whole group or not: four divisions in flight
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = flt ? __float_as_uint(dequantize1(bswap(w[u][t]), s)) : bswap(w[u][t]);
        E::store_group(out, g.j(u), n, v);
    }
}

}  // namespace sml

#endif  // SML_PACKET_PHASES_H_
