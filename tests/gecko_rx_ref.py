"""Restatement of Gecko's receive side (apernet/hysteria extras/obfs/gecko.go) with an
explicit millisecond clock, for the tests of the device receive path
(include/hyobfs_gecko.h: peek, reassembler, open).

TEST INFRASTRUCTURE ONLY.  The bytes come from oracle/salamander_ref.py and
oracle/gecko_ref.py; this file adds the state: ReadFrom, acceptChunk, gcExpired,
dropEntryLocked and evictOldestLocked.  Where the reference leaves a choice to Go's
map order (which of several entries with the same earliest deadline is evicted, the
order in which gcExpired drops), the rule of the header holds: the entry created
first goes first.

Two views of the same machine:
* ``Conn.read`` works on datagram bytes and returns what ReadFrom returns;
* ``Conn.feed`` works on what the C state machine sees (status, header, payload
  length, a tag) and returns what hyobfs_gecko_reassembler_feed returns.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from oracle import gecko_ref as G
from oracle import salamander_ref as S

TTL_MS = 8000              # geckoReassemblyTTL (gecko.go:21)
MAX_REASSEMBLY = 4096      # geckoMaxReassembly (gecko.go:24)
MAX_PER_SOURCE = 8         # geckoMaxPerSource (gecko.go:25)
PENDING, PASS, COMPLETE, DROPPED = 0, 1, 2, 3   # HYOBFS_GECKO_RX_*


@dataclass
class Entry:
    """reassemblyEntry (gecko.go:62-67); a chunk is (tag, payload or its length)."""
    total: int
    deadline: int
    seq: int
    chunks: list = field(default_factory=list)
    received: int = 0


class Conn:
    """The receive half of geckoPacketConn (gecko.go:69-81)."""

    def __init__(self):
        self.reassembly: dict[tuple[bytes, int], Entry] = {}
        self.per_source: dict[bytes, int] = {}
        self.released: list = []   # tags of the chunks of dropped entries (what Go's collector frees)
        self._seq = 0

    # ------------------------------------------------------------ gecko.go:169-197
    def read(self, psk: bytes, wire: bytes, addr, now_ms: int):
        """One turn of ReadFrom's loop over the Salamander conn below it: the payload
        returned for this wire datagram, or None where the loop continues."""
        plain = S.deobfuscate(psk, wire)           # salamander.go:74-86: b"" where it returns 0
        kind, h, payload = G.parse(plain)          # gecko.go:178-190
        if kind == G.PASS:
            return payload
        if kind != G.FRAGMENT:
            return None                            # n <= 0, or "malformed frame; drop silently"
        st, chunks = self.accept_chunk(str(addr).encode(), h.msg_id, h.chunk_idx, h.total_chunks, (None, payload), now_ms)
        return b"".join(p for _, p in chunks) if st == COMPLETE else None

    def feed(self, source: bytes, status: str, msg_id: int, idx: int, total: int, payload_len: int, tag, now_ms: int):
        """hyobfs_gecko_reassembler_feed: (code, tags, msg_len)."""
        if status == G.PASS:
            return PASS, [tag], payload_len
        if status != G.FRAGMENT or not G.MIN_CHUNKS <= total <= G.MAX_CHUNKS or idx >= total:
            return DROPPED, [], 0
        st, chunks = self.accept_chunk(source, msg_id, idx, total, (tag, payload_len), now_ms)
        if st != COMPLETE:
            return st, [], 0
        return st, [t for t, _ in chunks], min(sum(n for _, n in chunks), 0xFFFFFFFF)

    # ------------------------------------------------------------ gecko.go:199-249
    def accept_chunk(self, source: bytes, msg_id: int, idx: int, total: int, chunk, now_ms: int):
        key = (source, msg_id)
        e = self.reassembly.get(key)
        if e is None:
            if self.per_source.get(source, 0) >= MAX_PER_SOURCE:          # :207-210
                return DROPPED, None
            if len(self.reassembly) >= MAX_REASSEMBLY:                    # :211-214
                self.evict_oldest()
            e = Entry(total, now_ms + TTL_MS, self._seq, [None] * total)  # :215-219: set once, never refreshed
            self._seq += 1
            self.reassembly[key] = e
            self.per_source[source] = self.per_source.get(source, 0) + 1
        elif e.total != total:                                            # :222-225
            return DROPPED, None
        if idx >= len(e.chunks) or e.chunks[idx] is not None:             # :226-229: the first copy wins
            return DROPPED, None
        e.chunks[idx] = chunk
        e.received += 1
        if e.received < e.total:                                          # :234-236
            return PENDING, None
        self.drop_entry(key, released=False)                              # :247
        return COMPLETE, e.chunks

    # ------------------------------------------------------------ gecko.go:266-274
    def gc_expired(self, now_ms: int) -> None:
        for k in sorted((k for k, e in self.reassembly.items() if now_ms > e.deadline),   # now.After: strict
                        key=lambda k: (self.reassembly[k].deadline, self.reassembly[k].seq)):
            self.drop_entry(k)

    # ------------------------------------------------------------ gecko.go:277-286
    def drop_entry(self, k, released: bool = True) -> None:
        e = self.reassembly.pop(k, None)
        if e is None:
            return
        if released:
            self.released += [c[0] for c in e.chunks if c is not None]
        self.per_source[k[0]] -= 1
        if self.per_source[k[0]] <= 0:
            del self.per_source[k[0]]

    # ------------------------------------------------------------ gecko.go:290-304
    def evict_oldest(self) -> None:
        if self.reassembly:
            self.drop_entry(min(self.reassembly, key=lambda k: (self.reassembly[k].deadline, self.reassembly[k].seq)))

    def take_released(self) -> list:
        out, self.released = self.released, []
        return out
