"""The UDP relay message and its fragmentation -- ``core/internal/protocol/proxy.go``
and ``core/internal/frag/frag.go`` on MI355X.

==================================================  ==================================================
reference (Go)                                      here
==================================================  ==================================================
``UDPMessage``, ``HeaderSize``, ``Size``,           ``UDPMessage`` (``header_size``, ``size``,
``Serialize`` (proxy.go:160-191)                    ``serialize``)
``ParseUDPMessage`` (:193-223)                      ``parse_udp_message`` and ``parse_batch`` (GPU)
``FragUDPMessage`` (frag.go:7-34)                   ``frag_udp_message``
``sendMessageAutoFrag`` (server/udp.go:218-235)     ``send_frags`` and ``frag_batch`` (GPU)
``Defragger`` (frag.go:40-80)                       ``Defragger`` (indices, on the host) and
                                                    ``assemble_batch`` (GPU: the copy)
``ReceiveMessage`` -> ``Feed`` -> ``Hook``          ``relay_quic_snis``
==================================================  ==================================================

``include/hyobfs_udpmsg.h`` states the rules and the traps.  Everything runs in
``libhyobfs.so``; there is no Python path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, replace

import numpy as np

from . import _lib
from ._dev import _pack, _ptr, _records, _stream, _to

MAX_SIZE, MAX_ADDR, MAX_FRAGS = 4096, 2048, 255
(ERR_TRUNCATED, ERR_ADDR_LEN, ERR_MSG_LEN, ERR_FRAG_ID, TOO_LARGE, NO_ROOM, ERR_FRAG_COUNT, ERR_CAP,
 ERR_PLAN) = range(-68, -77, -1)
PENDING, WHOLE, COMPLETE = 0, 1, 2
ERRORS = {
    ERR_TRUNCATED: "truncated message",
    ERR_ADDR_LEN: "invalid address length",
    ERR_MSG_LEN: "invalid message length",
    ERR_FRAG_ID: "fragment id not below the fragment count",
    TOO_LARGE: "message larger than the send buffer (dropped)",
    NO_ROOM: "no room for a payload byte after the header",
    ERR_FRAG_COUNT: "more than 255 fragments",
    ERR_CAP: "output too small",
    ERR_PLAN: "fragment list cannot be assembled",
}


class UDPMessageError(ValueError):
    def __init__(self, status: int):
        self.status = status
        super().__init__(f"{ERRORS.get(status, 'error')} ({status})")


class HyobfsUdpHeader(ctypes.Structure):
    """struct hyobfs_udp_header."""
    _fields_ = [("session_id", ctypes.c_uint32), ("packet_id", ctypes.c_uint16), ("frag_id", ctypes.c_uint8),
                ("frag_count", ctypes.c_uint8)]


class HyobfsUdpParsed(ctypes.Structure):
    """struct hyobfs_udp_parsed."""
    _fields_ = [("status", ctypes.c_int32), ("session_id", ctypes.c_uint32), ("packet_id", ctypes.c_uint16),
                ("frag_id", ctypes.c_uint8), ("frag_count", ctypes.c_uint8), ("addr_off", ctypes.c_uint32),
                ("addr_len", ctypes.c_uint32), ("data_off", ctypes.c_uint32), ("data_len", ctypes.c_uint32),
                ("reserved_", ctypes.c_uint32)]


class HyobfsUdpMeta(ctypes.Structure):
    """struct hyobfs_udp_meta."""
    _fields_ = [("session_id", ctypes.c_uint32), ("packet_id", ctypes.c_uint16), ("reserved_", ctypes.c_uint16),
                ("max_size", ctypes.c_uint32), ("addr_len", ctypes.c_uint32), ("addr_off", ctypes.c_uint64)]


PARSED_DTYPE = np.dtype([("status", "<i4"), ("session_id", "<u4"), ("packet_id", "<u2"), ("frag_id", "u1"),
                         ("frag_count", "u1"), ("addr_off", "<u4"), ("addr_len", "<u4"), ("data_off", "<u4"),
                         ("data_len", "<u4"), ("reserved_", "<u4")])
META_DTYPE = np.dtype([("session_id", "<u4"), ("packet_id", "<u2"), ("reserved_", "<u2"), ("max_size", "<u4"),
                       ("addr_len", "<u4"), ("addr_off", "<u8")])
UDP_PARSED_DTYPE, UDP_META_DTYPE = PARSED_DTYPE, META_DTYPE   # the package-level names
assert PARSED_DTYPE.itemsize == ctypes.sizeof(HyobfsUdpParsed) == 32
assert META_DTYPE.itemsize == ctypes.sizeof(HyobfsUdpMeta) == 24


def _ulib(lib=None):
    return _lib.declare(lib or _lib.load(), "udpmsg", _lib._UDP_SIG)


def _buf(b: bytes):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


# ------------------------------------------------------------------ host, scalar
@dataclass
class UDPMessage:
    session_id: int = 0
    packet_id: int = 0
    frag_id: int = 0
    frag_count: int = 0
    addr: bytes = b""
    data: bytes = b""

    def header_size(self) -> int:
        return int(_ulib().hyobfs_udp_header_size(len(self.addr)))

    def size(self) -> int:
        return self.header_size() + len(self.data)

    def serialize(self, cap: int = MAX_SIZE):
        """Serialize into a buffer of ``cap`` bytes: the bytes, or -1 when it is too small."""
        out = (ctypes.c_uint8 * max(cap, 1))()
        hdr = HyobfsUdpHeader(self.session_id, self.packet_id, self.frag_id, self.frag_count)
        addr, data = _buf(self.addr), _buf(self.data)
        n = _ulib().hyobfs_udp_serialize(ctypes.addressof(hdr), ctypes.addressof(addr), len(self.addr),
                                         ctypes.addressof(data), len(self.data), ctypes.addressof(out), cap)
        return -1 if n < 0 else bytes(out[:n])


def parse_record(msg: bytes) -> HyobfsUdpParsed:
    """hyobfs_udp_parse: the parsed record of one datagram (status included)."""
    r = HyobfsUdpParsed()
    b = _buf(msg)
    _ulib().hyobfs_udp_parse(ctypes.addressof(b), len(msg), ctypes.addressof(r))
    return r


def parse_udp_message(msg: bytes) -> UDPMessage:
    """ParseUDPMessage; UDPMessageError where the reference returns an error."""
    r = parse_record(msg)
    if r.status != _lib.HYOBFS_OK:
        raise UDPMessageError(r.status)
    return UDPMessage(r.session_id, r.packet_id, r.frag_id, r.frag_count, bytes(msg[r.addr_off:r.addr_off + r.addr_len]),
                      bytes(msg[r.data_off:r.data_off + r.data_len]))


def frag_plan(addr_len: int, data_len: int, max_size: int) -> tuple[int, int, int]:
    """hyobfs_udp_frag_plan: (status, count, max_payload)."""
    c, mp = ctypes.c_uint32(), ctypes.c_uint32()
    st = _ulib().hyobfs_udp_frag_plan(addr_len, data_len, max_size, ctypes.byref(c), ctypes.byref(mp))
    return st, c.value, mp.value


def frag_udp_message(m: UDPMessage, max_size: int) -> list[UDPMessage]:
    """FragUDPMessage: the fragments; [] where the reference returns nothing;
    UDPMessageError(ERR_FRAG_COUNT) where its uint8 count would wrap."""
    st, count, mp = frag_plan(len(m.addr), len(m.data), max_size)
    if st == NO_ROOM:
        return []
    if st != _lib.HYOBFS_OK:
        raise UDPMessageError(st)
    if count == 1:   # it fits: returned as it is
        return [replace(m)]
    return [replace(m, frag_id=k, frag_count=count, data=m.data[k * mp:(k + 1) * mp]) for k in range(count)]


def send_frags(session_id: int, packet_id: int, addr: bytes, data: bytes, max_size: int) -> tuple[int, list[bytes]]:
    """hyobfs_udp_send_frags (sendMessageAutoFrag for one message): (status, datagrams)."""
    lib = _ulib()
    meta = HyobfsUdpMeta(session_id, packet_id, 0, max_size, len(addr), 0)
    _, frags, _ = frag_plan(len(addr), len(data), max_size)
    cap = max(frags, 1) * int(lib.hyobfs_udp_header_size(len(addr))) + len(data)   # what rule F needs, if it produces
    out = (ctypes.c_uint8 * cap)()
    lens = (ctypes.c_uint32 * MAX_FRAGS)()
    count = ctypes.c_uint32()
    a, d = _buf(addr), _buf(data)
    st = lib.hyobfs_udp_send_frags(ctypes.addressof(meta), ctypes.addressof(a), ctypes.addressof(d), len(data),
                                   ctypes.addressof(out), cap, ctypes.addressof(lens), ctypes.byref(count))
    ds, at = [], 0
    for k in range(count.value):
        ds.append(bytes(out[at:at + lens[k]]))
        at += lens[k]
    return st, ds


class Defragger:
    """Defragger.Feed over parsed records and the caller's tags (a datagram's batch
    index, say).  It keeps the reference's state, traps included."""

    def __init__(self):
        self._h = _ulib().hyobfs_udp_defragger_new()
        if not self._h:
            raise MemoryError("hyobfs_udp_defragger_new")
        self._tags = (ctypes.c_uint64 * MAX_FRAGS)()

    def feed(self, rec, tag: int) -> tuple[int, list[int]]:
        """(WHOLE | COMPLETE | PENDING | ERR_FRAG_ID, tags): ``rec`` is a HyobfsUdpParsed
        or a PARSED_DTYPE record; ``tags`` is in FragID order (empty unless WHOLE / COMPLETE)."""
        if not isinstance(rec, HyobfsUdpParsed):
            rec = HyobfsUdpParsed.from_buffer_copy(np.asarray(rec).tobytes())
        n = ctypes.c_uint32()
        st = _ulib().hyobfs_udp_defragger_feed(self._h, ctypes.addressof(rec), tag, ctypes.addressof(self._tags),
                                               ctypes.byref(n))
        if st == _lib.HYOBFS_ERR_INVALID:
            raise _lib.HyobfsError(st, "udp_defragger_feed")
        return st, list(self._tags[:n.value])

    def close(self):
        if getattr(self, "_h", None):
            _ulib().hyobfs_udp_defragger_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


# ------------------------------------------------------------------ device batches
def parse_batch(in_, in_off, in_len, n: int, out, stream=None) -> None:
    """hyobfs_udp_parse_batch: PARSED_DTYPE records of n device-resident datagrams."""
    _lib.check(_ulib().hyobfs_udp_parse_batch(_ptr(in_), _ptr(in_off), _ptr(in_len), n, _ptr(out), _stream(stream, out)),
               "udp_parse_batch")


def frag_workspace_size(n: int) -> int:
    return int(_ulib().hyobfs_udp_frag_workspace_size(n))


def frag_batch(data, data_off, data_len, meta, addrs, n: int, out, out_cap: int, dgram_off, dgram_len, dgram_cap: int,
               first, status, totals, workspace, stream=None) -> None:
    """hyobfs_udp_frag_batch: sendMessageAutoFrag over n device-resident messages."""
    st = _ulib().hyobfs_udp_frag_batch(_ptr(data), _ptr(data_off), _ptr(data_len), _ptr(meta), _ptr(addrs), n, _ptr(out),
                                       out_cap, _ptr(dgram_off), _ptr(dgram_len), dgram_cap, _ptr(first), _ptr(status),
                                       _ptr(totals), _ptr(workspace), _stream(stream, status))
    _lib.check(st, "udp_frag_batch")


def assemble_batch(in_, in_off, parsed, n: int, frag_idx, msg_first, m: int, out, out_off, out_cap, out_len, status,
                   stream=None) -> None:
    """hyobfs_udp_assemble_batch: the data of m messages, each the concatenation of
    the data slices of the datagrams its list names."""
    st = _ulib().hyobfs_udp_assemble_batch(_ptr(in_), _ptr(in_off), _ptr(parsed), n, _ptr(frag_idx), _ptr(msg_first), m,
                                           _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                           _stream(stream, status))
    _lib.check(st, "udp_assemble_batch")


def defrag_plan(records):
    """The host half of the receive path: every OK record fed, in order, to the
    Defragger of its SessionID.  Returns (lists, last): per completed message
    the indices of its datagrams in FragID order, and the index of the datagram
    that completed it (whose SessionID and Addr the message carries, rule D5)."""
    defraggers: dict[int, Defragger] = {}
    lists, last = [], []
    try:
        for i, r in enumerate(records):
            if r["status"] != _lib.HYOBFS_OK:
                continue   # server.go:371-374: an invalid message is skipped
            d = defraggers.get(int(r["session_id"]))
            if d is None:
                d = defraggers[int(r["session_id"])] = Defragger()
            st, tags = d.feed(r, i)
            if st in (WHOLE, COMPLETE):
                lists.append(tags)
                last.append(i)
    finally:
        for d in defraggers.values():
            d.close()
    return lists, last


def relay_quic_snis(datagrams, device: int = 0, name_stride: int = 255):
    """The receive path of relayed QUIC traffic on cuda:<device>: parse every
    datagram, defragment per SessionID, assemble the completed messages and sniff
    each one as a QUIC client Initial.  One server name (bytes), or None, per
    completed message, in completion order.  Only the 32-byte parsed records
    cross back to the host before the names."""
    import torch

    from . import quic, sniff
    dev = torch.device("cuda", device)
    n = len(datagrams)
    if n == 0:
        return []
    buf, off, lens = _pack(datagrams)
    d_in, d_off = _to(dev, buf), _to(dev, off)
    d_parsed = torch.zeros(n * PARSED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    parse_batch(d_in, d_off, _to(dev, lens), n, d_parsed)
    recs = _records(d_parsed, PARSED_DTYPE)
    lists, _ = defrag_plan(recs)
    m = len(lists)
    if m == 0:
        return []
    frag_idx = np.array([i for l in lists for i in l], np.uint32)
    msg_first = np.zeros(m + 1, np.uint64)
    np.cumsum([len(l) for l in lists], out=msg_first[1:])
    caps = np.array([sum(int(recs[i]["data_len"]) for i in l) for l in lists], np.uint32)
    out_off = np.zeros(m, np.uint64)
    np.cumsum(caps[:-1], out=out_off[1:])
    d_out = torch.zeros(int(caps.sum()) + 16, dtype=torch.uint8, device=dev)
    d_out_off = _to(dev, out_off)
    d_len = torch.zeros(m, dtype=torch.int32, device=dev)
    d_st = torch.zeros(m, dtype=torch.int32, device=dev)
    assemble_batch(d_in, d_off, d_parsed, n, _to(dev, frag_idx), _to(dev, msg_first), m, d_out, d_out_off,
                   _to(dev, caps), d_len, d_st)
    crypto_cap = max(4096, int(caps.max()))
    d_crypto = torch.zeros(m * crypto_cap, dtype=torch.uint8, device=dev)
    d_qres = torch.zeros(m * quic.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_names = torch.zeros(m * name_stride, dtype=torch.uint8, device=dev)
    d_sres = torch.zeros(m * sniff.SNIFF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(sniff.quic_sniff_workspace_size(m), 1), dtype=torch.uint8, device=dev)
    sniff.quic_sniff_batch(d_out, d_out_off, d_len, m, d_crypto,
                           _to(dev, np.arange(m, dtype=np.uint64) * np.uint64(crypto_cap)),
                           _to(dev, np.full(m, crypto_cap, np.uint32)), d_qres, d_names, name_stride, d_sres, ws)
    sres, names = _records(d_sres, sniff.SNIFF_RESULT_DTYPE), d_names.cpu().numpy()
    return [names[j * name_stride:j * name_stride + int(r["name_len"])].tobytes()
            if r["status"] == _lib.HYOBFS_OK and r["name_len"] else None for j, r in enumerate(sres)]
