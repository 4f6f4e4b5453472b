"""The wire format of a DPDK frame in Python, and the only Python module that
knows a byte offset of it: the twin of csrc/sml_frame_wire.h, written by hand
from the same table.  numpy only; the models, tests and tools the kernels are
held to, and anything that parses frames from a ring, name fields through it:

    FW.get(fr, FW.PKT_ID)     fr[..., FW.SRC_IP]     fr[..., FW.span(FW.DST_MAC, FW.IP_CHECKSUM)]

A frame is the last axis of whatever holds it: a 1-D array, a [F, stride] array
or a torch tensor.
"""
import socket

import numpy as np

BYTES, BE, LE = "bytes", "be", "le"        # as they are; an unsigned integer, big-endian; one in host order

# field: (first byte, last byte, encoding)
LAYOUT = {
    "DST_MAC": (0, 5, BYTES),
    "SRC_MAC": (6, 11, BYTES),
    "ETHERTYPE": (12, 13, BYTES),          # 08 00
    "IP_VER_TOS": (14, 15, BYTES),         # 45 00
    "IP_TOTAL_LEN": (16, 17, BE),
    "IP_ID_FRAG": (18, 21, BYTES),         # identification, flags / fragment: 0
    "IP_TTL": (22, 22, BE),                # a worker's 128, a result's 64
    "IP_PROTO": (23, 23, BE),              # UDP
    "IP_CHECKSUM": (24, 25, BE),           # a worker's 0
    "SRC_IP": (26, 29, BYTES),
    "DST_IP": (30, 33, BYTES),
    "SRC_PORT": (34, 35, BE),
    "DST_PORT": (36, 37, BE),
    "UDP_LEN": (38, 39, BE),
    "UDP_CHECKSUM": (40, 41, BYTES),       # a worker's pseudo-header sum in memory order, a result's 0
    "JOB_TYPE_SIZE": (42, 42, BE),         # 0x10 | size
    "JOB": (43, 43, BE),                   # short_job_id
    "PKT_ID": (44, 47, LE),                # pkt_id / tsi
    "POOL_INDEX": (48, 49, BE),            # slot in bits 0-13, set in bit 15
    "EXP": (50, 50, BE),
    "EXP2": (51, 51, BE),                  # a worker's 0
}
_ENCODING = {(lo, hi + 1): enc for lo, hi, enc in LAYOUT.values()}
# Every field as a slice of the last axis, in the table's order: DST_MAC = slice(0, 6), ..., EXP2 = slice(51, 52)
(DST_MAC, SRC_MAC, ETHERTYPE, IP_VER_TOS, IP_TOTAL_LEN, IP_ID_FRAG, IP_TTL, IP_PROTO, IP_CHECKSUM, SRC_IP, DST_IP,
 SRC_PORT, DST_PORT, UDP_LEN, UDP_CHECKSUM, JOB_TYPE_SIZE, JOB, PKT_ID, POOL_INDEX, EXP,
 EXP2) = (slice(lo, hi + 1) for lo, hi, _ in LAYOUT.values())


def span(first, last):
    """The bytes from field `first`'s start to field `last`'s end."""
    return slice(first.start, last.stop)


EXPS = span(EXP, EXP2)
IP_HEADER = span(IP_VER_TOS, DST_IP)
HEADER = span(DST_MAC, EXP2)
HEADER_BYTES = HEADER.stop
SWITCH_MAC, SWITCH_IP = bytes([2, 0, 0, 0, 0, 1]), "10.0.0.253"    # sml_frame_wire.h's example, worker_frame's default
POOL_BIT14 = 0x4000                        # of the pool index: neither slot nor set, a result has it cleared


def frame_bytes(P):
    return HEADER_BYTES + 4 * P


def payload(P):
    return slice(HEADER_BYTES, frame_bytes(P))


def ipv4_total_len(P):
    return frame_bytes(P) - IP_HEADER.start


def udp_len(P):
    return frame_bytes(P) - SRC_PORT.start


def job_type_size(P):
    return (1 << 4) + (0 if P < 64 else 1 if P < 128 else 2 if P < 256 else 3)


def _encoding(field):
    return _ENCODING.get((field.start, field.stop), BYTES)          # a span of fields is bytes


def _shifts(field):
    """The bit position of each of an integer field's bytes."""
    enc, n = _encoding(field), field.stop - field.start
    assert enc in (BE, LE), "not an integer field"
    return 8 * (np.arange(n) if enc == LE else np.arange(n)[::-1])


def get(f, field):
    """Field `field` (one of the slices above) of frame f, or of every frame
    of f's leading axes: an int (an integer array) by the field's encoding,
    bytes (the uint8 array) where it has none."""
    b = np.asarray(f[..., field])
    if _encoding(field) == BYTES:
        return bytes(b) if b.ndim == 1 else b
    v = (b.astype(np.int64) << _shifts(field)).sum(axis=-1)
    return int(v) if v.ndim == 0 else v


def put(f, field, value):
    """Write `value` (a scalar or one per frame; bytes or uint8 where the
    field has no encoding) as field `field` of f; no other byte changes."""
    if _encoding(field) == BYTES:
        b = np.frombuffer(value, np.uint8) if isinstance(value, (bytes, bytearray)) else np.asarray(value, np.uint8)
    else:
        b = ((np.asarray(value, dtype=np.int64)[..., None] >> _shifts(field)) & 0xff).astype(np.uint8)
    f[..., field] = b if isinstance(f, np.ndarray) else f.new_tensor(b)      # a torch tensor


def payload_words(f, P):
    """The payload's P words in host order (ntohl), uint32."""
    return np.ascontiguousarray(f[..., payload(P)]).view(">u4").astype(np.uint32)


def put_payload_words(f, P, words):
    """Write P host-order words as the payload (htonl)."""
    f[..., payload(P)] = np.asarray(words).astype(">u4").view(np.uint8)


def pool_index(pkt_id, mop, start=0, shift=0):
    """PktId2PoolIndex: slot (pkt_id + shift) % mop from `start`, the sets alternate per window."""
    i = (pkt_id + shift) % (2 * mop)
    return (start + i) & 0xffff if i < mop else ((start + i - mop) | 0x8000) & 0xffff


def pool_slot(idx):
    return idx & 0x3fff


def pool_set(idx):
    return idx >> 15


def ip_bytes(ip):
    """A dotted address (or its 4 bytes already) as the 4 bytes on the wire."""
    return socket.inet_aton(ip) if isinstance(ip, str) else bytes(ip)


def ip_be(ip):
    """The address as FrameParams holds it: the wire's bytes read as a host-order uint32."""
    return int.from_bytes(ip_bytes(ip), "little")


def ipv4_checksum(hdr20):
    """RFC 1071 over the 20 bytes of an IPv4 header (0 when its checksum is in place and right)."""
    s = 0
    for i in range(0, 20, 2):
        s += (int(hdr20[i]) << 8) | int(hdr20[i + 1])
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return ~s & 0xffff


def put_ipv4_header(f, P, ttl, src_ip, dst_ip):
    """The IPv4 header of a frame of P elements, its checksum left as it is (a worker's: 0)."""
    put(f, IP_VER_TOS, b"\x45\x00")
    put(f, IP_TOTAL_LEN, ipv4_total_len(P))
    put(f, IP_TTL, ttl)
    put(f, IP_PROTO, 17)
    put(f, SRC_IP, ip_bytes(src_ip))
    put(f, DST_IP, ip_bytes(dst_ip))


def result_ipv4_checksum(P, src_ip, dst_ip):
    """The header checksum of a result frame of P elements, as udp_sender fills the header."""
    f = np.zeros(HEADER_BYTES, dtype=np.uint8)
    put_ipv4_header(f, P, 64, src_ip, dst_ip)
    return ipv4_checksum(f[IP_HEADER])


def worker_frame(P, worker, pkt_id, pool_idx, payload, exps=(0, 0), src_port=4000, dst_port=48879, job=0,
                 switch_mac=SWITCH_MAC, switch_ip=SWITCH_IP):
    """A frame as BuildPacket lays it out, the UDP checksum left 0: `worker` =
    (mac, ip), payload = 4P wire bytes (uint8 array or bytes), exps = the
    two exponent bytes."""
    f = np.zeros(frame_bytes(P), dtype=np.uint8)
    put(f, DST_MAC, bytes(switch_mac))
    put(f, SRC_MAC, bytes(worker[0]))
    put(f, ETHERTYPE, b"\x08\x00")
    put_ipv4_header(f, P, 128, worker[1], switch_ip)
    put(f, SRC_PORT, src_port)
    put(f, DST_PORT, dst_port)
    put(f, UDP_LEN, udp_len(P))
    put(f, JOB_TYPE_SIZE, job_type_size(P))
    put(f, JOB, job & 0xff)
    put(f, PKT_ID, pkt_id)
    put(f, POOL_INDEX, pool_idx)
    put(f, EXPS, [exps[0] & 0xff, exps[1] & 0xff])
    f[HEADER_BYTES:] = np.frombuffer(bytes(payload), dtype=np.uint8) if not isinstance(payload, np.ndarray) else payload
    return f
