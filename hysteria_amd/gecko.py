"""Gecko shape obfuscation -- ``extras/obfs/gecko.go`` + ``gecko_frame.go`` on MI355X.

Gecko sits on top of a Salamander packet connection.  QUIC long-header
(handshake) packets are split into 2..8 chunks, each sent as its own frame
``0x80 | msgID | idx<<4|total | padLen | pad | chunk`` padded so the wire
datagram lands in ``[min_pkt, max_pkt]``; short-header packets pass through.

=============================================  ==============================================
reference (Go)                                 here
=============================================  ==============================================
``GeckoOptions`` (gecko.go:28-32)              ``GeckoOptions``
``WrapPacketConnGecko`` (gecko.go:34-55)       ``wrap_packet_conn_gecko(sock, opts)``
``newGeckoPacketConn`` (gecko.go:83-95)        ``GeckoPacketConn(inner, min_pkt, max_pkt)``
``WriteTo`` / ``writeFragmented`` (:99-129)    ``write_to(p, addr)``
``ReadFrom`` / ``acceptChunk`` (:157-250)      ``read_from(bufsize)`` / ``accept_chunk``
``gcLoop`` / ``gcExpired`` (:254-275)          background thread / ``gc_expired(now)``
``evictOldestLocked`` (:291-307)               ``evict_oldest_locked()``
``encodeFrame`` / ``decodeFrame``              ``encode_frame`` / ``decode_frame`` (C ABI)
``randomPadLen`` / ``randIntn`` (:131-153)     ``random_pad_len`` / ``rand_intn``
(new) one device pass over many frames         ``plan_fragments`` + ``encode_batch`` (GPU)
(new) device parse of received datagrams       ``parse_batch`` (GPU)
(new) the receive side without the padding     ``peek_batch`` (GPU), ``Reassembler`` (the C
                                               state machine over indices), ``open_batch``
                                               (GPU); ``GeckoReceiver`` runs the three
=============================================  ==============================================

The frame codec and the device batch calls go through ``include/hyobfs_gecko.h``
(``libhyobfs.so``); the reassembly table stays on the host, as in the reference.
"""
from __future__ import annotations

import ctypes
import os
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._dev import _ptr, _stream, _to
from ._lib import _i32, _i64, _sz, _u32, _u64, _vp, check

FLAG_FRAGMENT = 0x80
HEADER_LEN = 5
MIN_FRAGMENT_CHUNKS = 2
MAX_FRAGMENT_CHUNKS = 8
REASSEMBLY_TTL = 8.0          # seconds
MAX_REASSEMBLY = 4096
MAX_PER_SOURCE = 8
BUFFER_SIZE = 2048
DEFAULT_MIN_PACKET = 512
DEFAULT_MAX_PACKET = 1200
SALT_LEN = 8

ERR_TRUNCATED = -20
ERR_INVALID = -21
PASS, FRAGMENT, EMPTY = 0, 1, -22
ERR_CAP, ERR_PLAN = -23, -24                          # open_batch, per message
RX_PENDING, RX_PASS, RX_COMPLETE, RX_DROPPED = 0, 1, 2, 3   # Reassembler.feed
REASSEMBLY_TTL_MS = 8000


class FrameTruncatedError(ValueError):
    """errFrameTruncated (gecko_frame.go:19)."""


class FrameInvalidError(ValueError):
    """errFrameInvalid (gecko_frame.go:20)."""


class GeckoError(ValueError):
    """Construction errors of WrapPacketConnGecko (gecko.go:35-47)."""


class UnsupportedError(OSError):
    """errors.ErrUnsupported: the inner conn is not UDP-like (gecko.go:320-341)."""


class HyobfsGeckoHeader(ctypes.Structure):
    _fields_ = [("pad_len", ctypes.c_uint16), ("msg_id", ctypes.c_uint8), ("chunk_idx", ctypes.c_uint8),
                ("total_chunks", ctypes.c_uint8), ("reserved_", ctypes.c_uint8 * 3)]


class HyobfsGeckoBatch(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("msg", ctypes.c_void_p), ("frames", ctypes.c_void_p),
                ("salts", ctypes.c_void_p), ("pad_key", ctypes.c_uint8 * 32), ("pad_nonce", ctypes.c_uint8 * 12),
                ("reserved_", ctypes.c_uint32), ("out", ctypes.c_void_p),
                ("out_off", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_uint64),
                ("out_cap", ctypes.c_uint64)]


# struct hyobfs_gecko_frame / hyobfs_gecko_parsed as numpy records (16 bytes each)
FRAME_DTYPE = np.dtype([("chunk_off", "<u8"), ("chunk_len", "<u4"), ("pad_len", "<u2"), ("msg_id", "u1"),
                        ("idx_total", "u1")])
PARSED_DTYPE = np.dtype([("status", "<i4"), ("pad_len", "<u2"), ("msg_id", "u1"), ("idx_total", "u1"),
                         ("payload_off", "<u4"), ("payload_len", "<u4")])
assert FRAME_DTYPE.itemsize == 16 and PARSED_DTYPE.itemsize == 16


_hp = ctypes.POINTER(HyobfsGeckoHeader)
_SIG = {   # include/hyobfs_gecko.h
    "hyobfs_gecko_encode_frame": (_i64, [_hp, _vp, _sz, _vp, _sz]),
    "hyobfs_gecko_decode_frame": (_i32, [_vp, _sz, _hp, ctypes.POINTER(_sz)]),
    "hyobfs_gecko_pad_len": (_u32, [_i32, _i32, _u32, _u32]),
    "hyobfs_gecko_workspace_size": (_u64, [_u64]),
    "hyobfs_gecko_encode_batch": (_i32, [_vp, ctypes.POINTER(HyobfsGeckoBatch), _vp]),
    "hyobfs_gecko_parse_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "hyobfs_gecko_random_pad_key": (_i32, [_vp, _vp]),
    "hyobfs_gecko_peek_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "hyobfs_gecko_open_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hyobfs_gecko_reassembler_new": (_vp, []),
    "hyobfs_gecko_reassembler_free": (None, [_vp]),
    "hyobfs_gecko_reassembler_feed": (_i32, [_vp, _vp, _u32, _vp, _u64, _u64, _vp, ctypes.POINTER(_u32),
                                             ctypes.POINTER(_u32)]),
    "hyobfs_gecko_reassembler_gc": (None, [_vp, _u64]),
    "hyobfs_gecko_reassembler_pending": (_u64, [_vp]),
    "hyobfs_gecko_reassembler_released": (_u64, [_vp, _vp, _u64]),
}


def _glib(lib=None):
    return _lib.declare(lib or _lib.load(), "gecko", _SIG)


@dataclass(frozen=True)
class FrameHeader:
    """frameHeader (gecko_frame.go:30-35)."""
    pad_len: int
    msg_id: int
    chunk_idx: int
    total_chunks: int


def encode_frame(h: FrameHeader, payload: bytes, cap: int | None = None) -> bytes:
    """encodeFrame (gecko_frame.go:39-61): header, pad_len random bytes, payload."""
    payload = bytes(payload)
    need = HEADER_LEN + h.pad_len + len(payload)
    cap = need if cap is None else cap
    out = ctypes.create_string_buffer(max(cap, 1))
    ch = HyobfsGeckoHeader(pad_len=h.pad_len, msg_id=h.msg_id & 0xFF, chunk_idx=h.chunk_idx & 0xFF,
                           total_chunks=h.total_chunks & 0xFF)
    r = _glib().hyobfs_gecko_encode_frame(ctypes.byref(ch), payload, len(payload), out, cap)
    if r == ERR_INVALID:
        raise FrameInvalidError("gecko frame invalid")
    if r == ERR_TRUNCATED:
        raise FrameTruncatedError("gecko frame truncated")
    check(int(r) if r < 0 else 0, "encode_frame")
    return out.raw[:r]


def decode_frame(buf: bytes) -> tuple[FrameHeader, bytes]:
    """decodeFrame (gecko_frame.go:65-86): (header, payload)."""
    buf = bytes(buf)
    h = HyobfsGeckoHeader()
    off = ctypes.c_size_t()
    r = _glib().hyobfs_gecko_decode_frame(buf, len(buf), ctypes.byref(h), ctypes.byref(off))
    if r == ERR_INVALID:
        raise FrameInvalidError("gecko frame invalid")
    if r == ERR_TRUNCATED:
        raise FrameTruncatedError("gecko frame truncated")
    check(r, "decode_frame")
    return FrameHeader(h.pad_len, h.msg_id, h.chunk_idx, h.total_chunks), buf[off.value:]


def rand_intn(n: int) -> int:
    """randIntn (gecko.go:145-153): uniform in [0, n) from 4 random bytes, big-endian, mod n."""
    if n <= 1:
        return 0
    return int.from_bytes(os.urandom(4), "big") % n


def random_fragment_chunks() -> int:
    """randomFragmentChunks (gecko.go:140-142)."""
    return MIN_FRAGMENT_CHUNKS + rand_intn(MAX_FRAGMENT_CHUNKS - MIN_FRAGMENT_CHUNKS + 1)


def random_pad_len(min_pkt: int, max_pkt: int, chunk_len: int) -> int:
    """randomPadLen (gecko.go:131-138), through the C ABI with 4 random bytes."""
    return int(_glib().hyobfs_gecko_pad_len(min_pkt, max_pkt, chunk_len, int.from_bytes(os.urandom(4), "big")))


def chunk_bounds(msg_len: int, chunks: int) -> list[tuple[int, int]]:
    """writeFragmented's chunking (gecko.go:109-118): len/chunks each, the last takes the rest."""
    size = msg_len // chunks
    return [(i * size, msg_len if i == chunks - 1 else (i + 1) * size) for i in range(chunks)]


@dataclass
class GeckoOptions:
    """GeckoOptions (gecko.go:28-32)."""
    password: bytes = b""
    min_packet_size: int = 0
    max_packet_size: int = 0


def _validate(opts: GeckoOptions) -> tuple[int, int]:
    if not opts.password:
        raise GeckoError("gecko: password is required")
    lo = opts.min_packet_size or DEFAULT_MIN_PACKET
    hi = opts.max_packet_size or DEFAULT_MAX_PACKET
    if lo <= 0 or lo > hi or hi > BUFFER_SIZE:
        raise GeckoError("gecko: invalid min/max packet size")
    return lo, hi


@dataclass
class _Entry:
    chunks: list
    received: int
    total: int
    deadline: float


class GeckoPacketConn:
    """geckoPacketConn (gecko.go:69-95) over an inner packet conn with
    ``write_to(p, addr)`` / ``read_from(bufsize) -> (payload, addr)`` / ``close()``."""

    def __init__(self, inner, min_pkt: int = DEFAULT_MIN_PACKET, max_pkt: int = DEFAULT_MAX_PACKET):
        self.inner = inner
        self.min_pkt, self.max_pkt = min_pkt, max_pkt
        self._msg_id = 0
        self._msg_lock = threading.Lock()
        self._read_lock = threading.Lock()
        self.mu = threading.Lock()
        self.reassembly: dict[tuple[str, int], _Entry] = {}
        self.per_source: dict[str, int] = {}
        self._closed = threading.Event()
        self._gc = threading.Thread(target=self._gc_loop, daemon=True)
        self._gc.start()

    # ---------------------------------------------------------------- send
    def write_to(self, p, addr) -> int:
        """WriteTo (gecko.go:99-110)."""
        p = bytes(p)
        if len(p) == 0:
            return 0
        if p[0] & 0x80:
            return self._write_fragmented(p, addr)
        return self.inner.write_to(p, addr)

    def _next_msg_id(self) -> int:
        with self._msg_lock:
            self._msg_id = (self._msg_id + 1) & 0xFFFFFFFF
            return self._msg_id & 0xFF

    def _write_fragmented(self, p: bytes, addr) -> int:
        """writeFragmented (gecko.go:112-129)."""
        chunks = random_fragment_chunks()
        msg_id = self._next_msg_id()
        for i, (s, e) in enumerate(chunk_bounds(len(p), chunks)):
            chunk = p[s:e]
            pad = random_pad_len(self.min_pkt, self.max_pkt, len(chunk))
            frame = encode_frame(FrameHeader(pad, msg_id, i, chunks), chunk)
            self.inner.write_to(frame, addr)
        return len(p)

    # ------------------------------------------------------------- receive
    def read_from(self, bufsize: int = BUFFER_SIZE):
        """ReadFrom (gecko.go:157-193): returns (payload, addr)."""
        with self._read_lock:
            while True:
                buf, addr = self.inner.read_from(BUFFER_SIZE)
                if len(buf) <= 0:
                    continue
                if not buf[0] & 0x80:
                    return bytes(buf[:bufsize]), addr
                try:
                    h, payload = decode_frame(buf)
                except (FrameTruncatedError, FrameInvalidError):
                    continue   # malformed frame: dropped silently
                out = self.accept_chunk(addr, h, payload)
                if out is None:
                    continue
                return out[:bufsize], addr

    def accept_chunk(self, addr, h: FrameHeader, payload: bytes):
        """acceptChunk (gecko.go:195-250): the reassembled message, or None."""
        key = (str(addr), h.msg_id)
        with self.mu:
            e = self.reassembly.get(key)
            if e is None:
                if self.per_source.get(key[0], 0) >= MAX_PER_SOURCE:
                    return None
                if len(self.reassembly) >= MAX_REASSEMBLY:
                    self.evict_oldest_locked()
                e = _Entry([None] * h.total_chunks, 0, h.total_chunks, time.monotonic() + REASSEMBLY_TTL)
                self.reassembly[key] = e
                self.per_source[key[0]] = self.per_source.get(key[0], 0) + 1
            elif e.total != h.total_chunks:
                return None   # inconsistent chunk count
            if h.chunk_idx >= len(e.chunks) or e.chunks[h.chunk_idx] is not None:
                return None   # bad index or duplicate
            e.chunks[h.chunk_idx] = bytes(payload)
            e.received += 1
            if e.received < e.total:
                return None
            out = b"".join(e.chunks)
            self.drop_entry_locked(key)
            return out

    # --------------------------------------------------------- maintenance
    def _gc_loop(self) -> None:
        while not self._closed.wait(REASSEMBLY_TTL / 2):
            self.gc_expired(time.monotonic())

    def gc_expired(self, now: float) -> None:
        """gcExpired (gecko.go:265-275); ``now`` on the time.monotonic() clock."""
        with self.mu:
            for k in [k for k, e in self.reassembly.items() if now > e.deadline]:
                self.drop_entry_locked(k)

    def drop_entry_locked(self, k) -> None:
        if self.reassembly.pop(k, None) is None:
            return
        n = self.per_source.get(k[0], 0) - 1
        if n <= 0:
            self.per_source.pop(k[0], None)
        else:
            self.per_source[k[0]] = n

    def evict_oldest_locked(self) -> None:
        """evictOldestLocked (gecko.go:291-307): drop the entry with the earliest deadline."""
        if self.reassembly:
            k = min(self.reassembly, key=lambda k: self.reassembly[k].deadline)
            self.drop_entry_locked(k)

    # ---------------------------------------------------------- boilerplate
    def close(self) -> None:
        self._closed.set()
        if self.inner is not None:
            self.inner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def local_addr(self):
        return self.inner.local_addr()

    def _udp(self, name):
        f = getattr(self.inner, name, None)
        if f is None:
            raise UnsupportedError("unsupported operation")
        return f

    def fileno(self) -> int:
        return self._udp("fileno")()

    def set_read_buffer(self, nbytes: int) -> None:
        self._udp("set_read_buffer")(nbytes)

    def set_write_buffer(self, nbytes: int) -> None:
        self._udp("set_write_buffer")(nbytes)


def wrap_packet_conn_gecko(sock, opts: GeckoOptions, device: int = 0) -> GeckoPacketConn:
    """WrapPacketConnGecko (gecko.go:34-55): options checked before any device work."""
    lo, hi = _validate(opts)
    from .conn import wrap_packet_conn_salamander
    inner = wrap_packet_conn_salamander(sock, opts.password, device)
    return GeckoPacketConn(inner, lo, hi)


# ------------------------------------------------------------- device batches
def plan_fragments(msg_lens, min_pkt: int = DEFAULT_MIN_PACKET, max_pkt: int = DEFAULT_MAX_PACKET,
                   first_msg_id: int = 1, rand32=None):
    """Frames for a batch of long-header messages laid back to back in one buffer,
    as writeFragmented would send them (gecko.go:112-129).

    rand32(k) -> k uniform uint32 values (default: os.urandom).  Returns
    (frames: FRAME_DTYPE array, out_off: uint64 array of packed wire offsets, total wire bytes)."""
    if rand32 is None:
        def rand32(k):
            return np.frombuffer(os.urandom(4 * k), ">u4").astype(np.uint64)
    lib = _glib()
    frames = []
    off = 0
    for m, L in enumerate(msg_lens):
        r = rand32(1 + MAX_FRAGMENT_CHUNKS)
        chunks = MIN_FRAGMENT_CHUNKS + int(r[0] % (MAX_FRAGMENT_CHUNKS - MIN_FRAGMENT_CHUNKS + 1))
        mid = (first_msg_id + m) & 0xFF
        for i, (s, e) in enumerate(chunk_bounds(int(L), chunks)):
            pad = int(lib.hyobfs_gecko_pad_len(min_pkt, max_pkt, e - s, int(r[1 + i])))
            frames.append((off + s, e - s, pad, mid, (i << 4) | chunks))
        off += int(L)
    fr = np.array(frames, dtype=FRAME_DTYPE)
    widths = SALT_LEN + HEADER_LEN + fr["pad_len"].astype(np.uint64) + fr["chunk_len"].astype(np.uint64)
    out_off = np.zeros(len(fr), np.uint64)
    if len(fr):
        np.cumsum(widths[:-1], out=out_off[1:])
    return fr, out_off, int(widths.sum())


def workspace_size(n: int) -> int:
    return int(_glib().hyobfs_gecko_workspace_size(n))


def random_pad_key() -> tuple[bytes, bytes]:
    """A fresh (key, nonce) for the padding keystream from the OS (hyobfs_gecko_random_pad_key,
    getrandom: the source of the reference's crypto/rand)."""
    key, nonce = ctypes.create_string_buffer(32), ctypes.create_string_buffer(12)
    check(_glib().hyobfs_gecko_random_pad_key(key, nonce), "random_pad_key")
    return key.raw, nonce.raw


def encode_batch(obfuscator, *, msg, frames, salts, out, out_off, pad_key: bytes | None = None,
                 pad_nonce: bytes | None = None, workspace=None, n=None, stream=None) -> None:
    """hyobfs_gecko_encode_batch: every frame's wire datagram in one device pass.
    Arguments are device tensors (torch) or device pointers; ``workspace`` is accepted
    and ignored (ABI 3: no scratch).  Padding is a keyed keystream
    (include/hyobfs_gecko.h): a fresh OS-random key per call unless pad_key and
    pad_nonce are given (reproducible output for tests)."""
    if n is None:   # frames: 16-byte hyobfs_gecko_frame records
        n = frames.numel() * frames.element_size() // FRAME_DTYPE.itemsize if hasattr(frames, "numel") else len(frames)
    if pad_key is None or pad_nonce is None:
        pad_key, pad_nonce = random_pad_key()
    if len(pad_key) != 32 or len(pad_nonce) != 12:
        raise ValueError("pad_key must be 32 bytes and pad_nonce 12")
    b = HyobfsGeckoBatch(n=n, msg=_ptr(msg), frames=_ptr(frames), salts=_ptr(salts),
                         pad_key=(ctypes.c_uint8 * 32).from_buffer_copy(pad_key),
                         pad_nonce=(ctypes.c_uint8 * 12).from_buffer_copy(pad_nonce),
                         out=_ptr(out), out_off=_ptr(out_off))
    lib = _glib(getattr(obfuscator, "_lib", None))   # the library the context came from
    check(lib.hyobfs_gecko_encode_batch(obfuscator._h, ctypes.byref(b), _stream(stream, out)), "gecko_encode_batch")


def parse_batch(inp, in_off, in_len, n: int, out, stream=None) -> None:
    """hyobfs_gecko_parse_batch: classify n deobfuscated device datagrams into ``out``
    (PARSED_DTYPE records, 16 bytes each)."""
    check(_glib().hyobfs_gecko_parse_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), n, _ptr(out),
                                           _stream(stream, out)), "gecko_parse_batch")


# ------------------------------------------------- receive side without the padding
def peek_batch(obfuscator, wire, wire_off, wire_len, n: int, parsed, keys, stream=None) -> None:
    """hyobfs_gecko_peek_batch: for n still obfuscated device datagrams, the Salamander
    key (32 bytes each into ``keys``) and the PARSED_DTYPE record of the plaintext, read
    from the salt and at most five bytes behind it."""
    lib = _glib(getattr(obfuscator, "_lib", None))
    check(lib.hyobfs_gecko_peek_batch(obfuscator._h, _ptr(wire), _ptr(wire_off), _ptr(wire_len), n, _ptr(parsed),
                                      _ptr(keys), _stream(stream, parsed)), "gecko_peek_batch")


def open_batch(wire, wire_off, wire_len, parsed, keys, n: int, chunk_idx, msg_first, m: int, out, out_off, out_cap,
               out_len, status, stream=None) -> None:
    """hyobfs_gecko_open_batch: m messages, each the deobfuscated payloads of the slots
    its list names (a table of n slots as peek_batch left them), concatenated."""
    check(_glib().hyobfs_gecko_open_batch(_ptr(wire), _ptr(wire_off), _ptr(wire_len), _ptr(parsed), _ptr(keys), n,
                                          _ptr(chunk_idx), _ptr(msg_first), m, _ptr(out), _ptr(out_off), _ptr(out_cap),
                                          _ptr(out_len), _ptr(status), _stream(stream, status)), "gecko_open_batch")


class Reassembler:
    """hyobfs_gecko_reassembler: acceptChunk, gcExpired and evictOldestLocked
    (gecko.go:199-304) over parsed records and the caller's tags, on the caller's
    millisecond clock.  It never sees a payload."""

    def __init__(self):
        self._h = _glib().hyobfs_gecko_reassembler_new()
        if not self._h:
            raise MemoryError("hyobfs_gecko_reassembler_new")
        self._tags = (ctypes.c_uint64 * MAX_FRAGMENT_CHUNKS)()

    def feed(self, source: bytes, rec, tag: int, now_ms: int) -> tuple[int, list[int], int]:
        """(RX_PENDING | RX_PASS | RX_COMPLETE | RX_DROPPED, tags, msg_len): ``rec`` is a
        PARSED_DTYPE record (or its 16 bytes); ``tags`` is in chunk order, empty unless
        RX_PASS / RX_COMPLETE."""
        raw = rec if isinstance(rec, (bytes, bytearray)) else np.asarray(rec).tobytes()
        n, ln = ctypes.c_uint32(), ctypes.c_uint32()
        st = _glib().hyobfs_gecko_reassembler_feed(self._h, source, len(source), raw, tag, now_ms,
                                                   ctypes.addressof(self._tags), ctypes.byref(n), ctypes.byref(ln))
        if st < 0:
            raise _lib.HyobfsError(st, "gecko_reassembler_feed")
        return st, list(self._tags[:n.value]), ln.value

    def gc(self, now_ms: int) -> None:
        _glib().hyobfs_gecko_reassembler_gc(self._h, now_ms)

    def pending(self) -> int:
        return int(_glib().hyobfs_gecko_reassembler_pending(self._h))

    def released(self) -> list[int]:
        """The tags of chunks dropped by gc or eviction since the last call, oldest first."""
        lib = _glib()
        k = int(lib.hyobfs_gecko_reassembler_released(self._h, None, 0))
        if k == 0:
            return []
        buf = (ctypes.c_uint64 * k)()
        return list(buf[:lib.hyobfs_gecko_reassembler_released(self._h, ctypes.addressof(buf), k)])

    def close(self) -> None:
        if getattr(self, "_h", None):
            _glib().hyobfs_gecko_reassembler_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


class GeckoReceiver:
    """The receive pipeline on the obfuscator's device: wire datagrams in, what a
    sequence of ReadFrom calls (gecko.go:169-197) returns out.

    Received datagrams stay on the device, still obfuscated, in a table of
    ``BUFFER_SIZE``-byte slots until their message is complete; only the 16-byte
    records cross to the host, and only payload bytes are ever deobfuscated.  The
    table has ``MAX_REASSEMBLY * (MAX_FRAGMENT_CHUNKS - 1) + max_batch`` slots: every
    pending entry lacks at least one chunk, so it cannot run out."""

    def __init__(self, obfuscator, max_batch: int = 64):
        import torch
        self._o, self.max_batch = obfuscator, max_batch
        self._dev = dev = torch.device("cuda", obfuscator.device)
        self.slots = S = MAX_REASSEMBLY * (MAX_FRAGMENT_CHUNKS - 1) + max_batch
        self._wire = torch.zeros((S, BUFFER_SIZE), dtype=torch.uint8, device=dev)
        self._off = torch.arange(S, dtype=torch.int64, device=dev) * BUFFER_SIZE
        self._len = torch.zeros(S, dtype=torch.int32, device=dev)
        self._parsed = torch.zeros((S, PARSED_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        self._keys = torch.zeros((S, 32), dtype=torch.uint8, device=dev)
        self._free = list(range(S - 1, -1, -1))   # a stack: slot 0 first
        self._pinned: set[int] = set()            # slots of chunks that wait for the rest of their message
        self._r = Reassembler()

    @property
    def free_slots(self) -> int:
        return len(self._free)

    @property
    def pinned_slots(self) -> int:
        return len(self._pinned)

    def pending(self) -> int:
        return self._r.pending()

    def gc(self, now_ms: int) -> None:
        """gcExpired; the slots of the dropped chunks are free again."""
        self._r.gc(now_ms)
        self._release()

    def _release(self) -> None:
        for t in self._r.released():
            self._pinned.discard(t)
            self._free.append(t)

    def push(self, datagrams, addrs, now_ms: int):
        """Wire datagrams (bytes, as read from the socket) and their source addresses,
        in arrival order; returns [(payload, addr), ...] in the order of the datagrams
        that produced them, each with the address of the datagram that completed it.
        A datagram longer than BUFFER_SIZE is cut there, as the read buffer cuts it."""
        out = []
        for at in range(0, len(datagrams), self.max_batch):
            out += self._push(datagrams[at:at + self.max_batch], addrs[at:at + self.max_batch], now_ms)
        return out

    def _push(self, datagrams, addrs, now_ms):
        import torch
        n, dev = len(datagrams), self._dev
        if n == 0:
            return []
        slots = [self._free.pop() for _ in range(n)]
        fed, done = 0, []   # datagrams handed to the reassembler; slots to free when this push is over
        try:
            datagrams = [bytes(d)[:BUFFER_SIZE] for d in datagrams]
            lens = np.array([len(d) for d in datagrams], np.int32)
            width = max(16, -(-int(lens.max()) // 16) * 16)   # the rows go up as wide as the longest datagram
            rows = np.zeros((n, width), np.uint8)
            for i, d in enumerate(datagrams):
                rows[i, :len(d)] = np.frombuffer(d, np.uint8)
            idx = torch.from_numpy(np.array(slots, np.int64)).to(dev)
            d_lens = torch.from_numpy(lens).to(dev)
            self._wire[:, :width].index_copy_(0, idx, torch.from_numpy(rows).to(dev))   # straight into their slots
            self._len.index_copy_(0, idx, d_lens)
            # peek over the slots; it numbers its outputs by datagram, the table by slot
            d_parsed = torch.empty((n, PARSED_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            d_keys = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
            peek_batch(self._o, self._wire, self._off[idx], d_lens, n, d_parsed, d_keys)
            self._parsed.index_copy_(0, idx, d_parsed)
            self._keys.index_copy_(0, idx, d_keys)
            recs = np.frombuffer(d_parsed.cpu().numpy().tobytes(), PARSED_DTYPE)
            lists, caps, who = [], [], []
            for i, slot in enumerate(slots):
                st, tags, msg_len = self._r.feed(str(addrs[i]).encode(), recs[i], slot, now_ms)
                fed = i + 1
                if st == RX_PENDING:
                    self._pinned.add(slot)
                elif st == RX_DROPPED:
                    done.append(slot)
                else:   # RX_PASS, RX_COMPLETE
                    lists.append(tags)
                    caps.append(msg_len)
                    who.append(addrs[i])
                    self._pinned.difference_update(tags)
                    done += tags
            if not lists:
                return []
            m = len(lists)
            msg_first = np.zeros(m + 1, np.uint64)
            np.cumsum([len(l) for l in lists], out=msg_first[1:])
            out_off = np.zeros(m, np.uint64)
            np.cumsum(np.array(caps[:-1], np.uint64), out=out_off[1:])
            d_out = torch.empty(int(sum(caps)) + 16, dtype=torch.uint8, device=dev)
            d_olen = torch.empty(m, dtype=torch.int32, device=dev)
            d_st = torch.empty(m, dtype=torch.int32, device=dev)
            open_batch(self._wire, self._off, self._len, self._parsed, self._keys, self.slots,
                       _to(dev, np.array([t for l in lists for t in l], np.uint32)), _to(dev, msg_first), m, d_out,
                       _to(dev, out_off), _to(dev, np.array(caps, np.uint32)), d_olen, d_st)
            h_st, h_out = d_st.cpu().numpy(), d_out.cpu().numpy()
            if h_st.any():   # cannot happen: the lists come from the reassembler, the caps from its sums
                raise _lib.HyobfsError(int(h_st[h_st != 0][0]), "gecko_open_batch")
            return [(h_out[int(o):int(o) + c].tobytes(), a) for o, c, a in zip(out_off, caps, who)]
        finally:   # also when a call raised: no slot is lost
            self._release()   # evictions of this push
            self._free += done + slots[fed:]

    def close(self) -> None:
        self._r.close()
