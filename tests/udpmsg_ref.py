"""A restatement of Hysteria's UDP relay message for the tests, written from the
Go text: core/internal/protocol/proxy.go:151-256 (UDPMessage, ParseUDPMessage,
varintPut), core/internal/frag/frag.go (FragUDPMessage, Defragger) and
core/server/udp.go:207-235 with server.go:387-402 (sendMessageAutoFrag,
SendMessage).  Test infrastructure only; it shares no code with the package.

The letters are those of include/hyobfs_udpmsg.h: S serialise, P parse, F
fragment, A send, D defragment.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

OK = 0
TRUNCATED, ADDR_LEN, MSG_LEN, FRAG_ID, TOO_LARGE, NO_ROOM, FRAG_COUNT, CAP, PLAN = range(-68, -77, -1)
PENDING, WHOLE, COMPLETE = 0, 1, 2
MAX_UDP_SIZE = 4096          # proxy.go:24
MAX_MESSAGE_LENGTH = 2048    # proxy.go:20
MAX_DATAGRAM_FRAME_SIZE = 1200   # proxy.go:23


def varint_len(v: int) -> int:
    """quicvarint.Len."""
    if v <= 63:
        return 1
    if v <= 16383:
        return 2
    if v <= 1073741823:
        return 4
    if v <= 4611686018427387903:
        return 8
    raise ValueError("does not fit into 62 bits")


def varint_put(v: int) -> bytes:
    """varintPut (proxy.go:227-256): the minimal form."""
    n = varint_len(v)
    return (v | {1: 0x00, 2: 0x40, 4: 0x80, 8: 0xC0}[n] << (8 * n - 8)).to_bytes(n, "big")


def varint_forms(v: int) -> list[bytes]:
    """Every encoding of v that quicvarint.Read accepts (the non-minimal ones too)."""
    return [(v | {1: 0x00, 2: 0x40, 4: 0x80, 8: 0xC0}[n] << (8 * n - 8)).to_bytes(n, "big")
            for n in (1, 2, 4, 8) if v < 1 << (8 * n - 2)]


@dataclass
class UDPMessage:
    session_id: int = 0
    packet_id: int = 0
    frag_id: int = 0
    frag_count: int = 0
    addr: bytes = b""
    data: bytes = b""

    def header_size(self) -> int:   # proxy.go:169-172
        return 4 + 2 + 1 + 1 + varint_len(len(self.addr)) + len(self.addr)

    def size(self) -> int:          # :174-176
        return self.header_size() + len(self.data)

    def serialize(self, cap: int):  # :178-191: the bytes, or -1 when the buffer is too small
        if cap < self.size():
            return -1
        return (self.session_id.to_bytes(4, "big") + self.packet_id.to_bytes(2, "big")
                + bytes([self.frag_id, self.frag_count]) + varint_put(len(self.addr)) + self.addr + self.data)


def parse(msg: bytes):
    """ParseUDPMessage (proxy.go:193-223): a UDPMessage, or the status of rule P."""
    if len(msg) < 8:                       # the four binary.Read calls
        return TRUNCATED
    if len(msg) < 9:                       # quicvarint.Read: no first byte
        return TRUNCATED
    n = 1 << (msg[8] >> 6)
    if len(msg) < 8 + n:
        return TRUNCATED
    l_addr = int.from_bytes(msg[8:8 + n], "big") & ((1 << (8 * n - 2)) - 1)
    if l_addr == 0 or l_addr > MAX_MESSAGE_LENGTH:
        return ADDR_LEN
    bs = msg[8 + n:]
    if len(bs) <= l_addr:
        return MSG_LEN
    return UDPMessage(int.from_bytes(msg[0:4], "big"), int.from_bytes(msg[4:6], "big"), msg[6], msg[7],
                      bytes(bs[:l_addr]), bytes(bs[l_addr:]))


def parsed_record(msg: bytes):
    """(status, session_id, packet_id, frag_id, frag_count, addr_off, addr_len, data_off, data_len)
    as struct hyobfs_udp_parsed holds them."""
    m = parse(msg)
    if not isinstance(m, UDPMessage):
        return (m, 0, 0, 0, 0, 0, 0, 0, 0)
    a_off = len(msg) - len(m.data) - len(m.addr)
    return (OK, m.session_id, m.packet_id, m.frag_id, m.frag_count, a_off, len(m.addr), a_off + len(m.addr),
            len(m.data))


def frag_plan(addr_len: int, data_len: int, max_size: int):
    """The arithmetic of FragUDPMessage: (status, count, max_payload)."""
    h = 8 + varint_len(addr_len) + addr_len
    if h + data_len <= max_size:
        return OK, 1, data_len
    mp = max_size - h
    if mp <= 0:
        return NO_ROOM, 0, 0
    count = (data_len + mp - 1) // mp
    if count > 255:      # the reference's uint8 wraps here and it then indexes out of range
        return FRAG_COUNT, 0, 0
    return OK, count, mp


def frag_udp_message(m: UDPMessage, max_size: int):
    """FragUDPMessage (frag.go:7-34): the fragments ([] for "nothing"), or FRAG_COUNT
    where the reference's uint8 count would wrap."""
    if m.size() <= max_size:
        return [replace(m)]
    full = m.data
    mp = max_size - m.header_size()
    if mp <= 0:
        return []
    count = (len(full) + mp - 1) // mp
    if count > 255:
        return FRAG_COUNT
    frags, off, frag_id = [], 0, 0
    while off < len(full):
        size = min(len(full) - off, mp)
        frags.append(replace(m, frag_id=frag_id, frag_count=count, data=full[off:off + size]))
        off += size
        frag_id += 1
    return frags


def send(session_id: int, packet_id: int, addr: bytes, data: bytes, max_size: int):
    """sendMessageAutoFrag over a connection whose SendDatagram refuses datagrams
    longer than max_size (udp.go:218-235, server.go:387-402): (status, datagrams)."""
    m = UDPMessage(session_id, 0, 0, 1, addr, data)
    if m.serialize(MAX_UDP_SIZE) == -1:     # A1: io.SendMessage drops it; err stays nil
        return TOO_LARGE, []
    if m.size() <= max_size:                # A2: SendDatagram succeeds
        return OK, [m.serialize(MAX_UDP_SIZE)]
    m.packet_id = packet_id                 # A3: DatagramTooLargeError
    frags = frag_udp_message(m, max_size)
    if frags == FRAG_COUNT:
        return FRAG_COUNT, []
    if not frags:
        return NO_ROOM, []
    return OK, [f.serialize(MAX_UDP_SIZE) for f in frags]


def send_batch(msgs, out_cap=None, dgram_cap=None):
    """hyobfs_udp_frag_batch's outputs for msgs = [(session_id, packet_id, addr, data, max_size)]:
    (status[n], first[n + 1], totals, datagrams of the written messages [(offset, bytes)])
    under the header's capacity rule.  None: no limit."""
    status, first, dgrams, nbytes, nd = [], [0], [], 0, 0
    for sid, pid, addr, data, max_size in msgs:
        st, ds = send(sid, pid, addr, data, max_size)
        b0, d0 = nbytes, nd
        nbytes += sum(len(d) for d in ds)
        nd += len(ds)
        if (out_cap is not None and nbytes > out_cap) or (dgram_cap is not None and nd > dgram_cap):
            st = CAP
        elif st == OK:
            for d in ds:
                dgrams.append((b0, d))
                b0 += len(d)
        status.append(st)
        first.append(nd)
    return status, first, (nbytes, nd), dgrams


class Defragger:
    """Defragger (frag.go:40-80).  feed() returns the message (whole or assembled) or None."""

    def __init__(self):
        self.pkt_id = 0
        self.frags: list = []
        self.count = 0

    def feed(self, m: UDPMessage):
        if m.frag_count <= 1:
            return m
        if m.frag_id >= m.frag_count:
            return None
        if m.packet_id != self.pkt_id or m.frag_count != len(self.frags):
            self.pkt_id = m.packet_id
            self.frags = [None] * m.frag_count
            self.frags[m.frag_id] = m
            self.count = 1
        elif self.frags[m.frag_id] is None:
            self.frags[m.frag_id] = m
            self.count += 1
            if self.count == len(self.frags):
                return replace(m, frag_id=0, frag_count=1, data=b"".join(f.data for f in self.frags))
        return None
