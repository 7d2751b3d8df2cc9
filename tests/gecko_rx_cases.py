"""The case lattices of Gecko's device receive path (include/hyobfs_gecko.h:
hyobfs_gecko_peek_batch, hyobfs_gecko_open_batch), shared by the CPU tier
(tests/test_gecko_rx.py through tests/emu/gecko_rx_main.cpp) and the GPU tier
(tests/test_gpu_gecko_rx.py).  TEST INFRASTRUCTURE ONLY.

A case is a table of wire datagrams at stated offsets of one buffer plus, for open,
the records and keys of the slots (computed here from the oracle, or forged), the
chunk lists and the output layout.  ``expected_peek`` / ``expected_open`` restate the
header's rules with oracle/salamander_ref.py and oracle/gecko_ref.py for the bytes.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import gecko_ref as gref
from oracle import salamander_ref as sref

GUARD = 0xA5      # what every output array holds before a call
FILL = 0xEE       # the bytes of a wire buffer that belong to no datagram
OUT_TAIL = 16     # guard bytes after the last message's output (before each: its gap)
PARSED_DTYPE = np.dtype([("status", "<i4"), ("pad_len", "<u2"), ("msg_id", "u1"), ("idx_total", "u1"),
                         ("payload_off", "<u4"), ("payload_len", "<u4")])
PASS, FRAGMENT, EMPTY, TRUNCATED, INVALID = 0, 1, -22, -20, -21
OK, ERR_CAP, ERR_PLAN = 0, -23, -24
STATUS = {gref.PASS: PASS, gref.FRAGMENT: FRAGMENT, gref.EMPTY: EMPTY, gref.TRUNCATED: TRUNCATED, gref.INVALID: INVALID}
PSK = b"average_password"
# every salt word of the one-block key, the last offsets of one block and the two-block case
PSK_LENS = (4, 9, 24, 57, 100, 113, 119, 120, 121, 127, 128, 200, 300)
PEEK_NS = (1, 63, 64, 65, 257)
OPEN_MS = (1, 3, 4, 5, 257)
OPEN_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 64, 600)


def psk_of(n: int) -> bytes:
    return bytes((11 * k + n) & 0xFF or 1 for k in range(n))


def _salt(i: int) -> bytes:
    return sref.splitmix64_at(7, i).to_bytes(8, "little")


def _fill(seed: int, n: int) -> bytes:
    return sref.stream_bytes(1000 + seed, 0, n)


def record(psk: bytes, wire: bytes) -> tuple:
    """The six fields hyobfs_gecko_peek_batch writes for one wire datagram:
    Deobfuscate (b"" where it returns 0), then ReadFrom's classification."""
    plain = sref.deobfuscate(psk, wire)
    kind, h, payload = gref.parse(plain)
    if kind == gref.PASS:
        return (PASS, 0, 0, 0, 0, len(plain))
    if kind == gref.FRAGMENT:
        return (FRAGMENT, h.pad_len, h.msg_id, h.chunk_idx << 4 | h.total_chunks, gref.HEADER_LEN + h.pad_len, len(payload))
    return (STATUS[kind], 0, 0, 0, 0, 0)


# ------------------------------------------------------------------ layouts
def packed(lens):
    """Back to back: the offsets take every residue the lengths give."""
    off = np.zeros(len(lens), np.uint64)
    if len(lens) > 1:
        np.cumsum(np.asarray(lens[:-1], np.uint64), out=off[1:])
    return off, int(sum(lens))


def slotted(lens):
    """8-aligned slots with at least one byte between two datagrams (poisoned on the CPU
    tier); the buffer ends with the last datagram."""
    off, at = [], 0
    for ln in lens:
        off.append(at)
        at += (ln + 8) // 8 * 8
    return np.array(off, np.uint64), (int(off[-1]) + lens[-1] if lens else 0)


def wire_buffer(case) -> np.ndarray:
    buf = np.full(max(case["buf_len"], 1), FILL, np.uint8)
    for o, w in zip(case["off"], case["wires"]):
        buf[int(o):int(o) + len(w)] = np.frombuffer(w, np.uint8)
    return buf[:case["buf_len"]]


# ------------------------------------------------------------------ peek
def _hdr(flag, msg_id, idx, total, pad):
    return bytes([flag, msg_id & 0xFF, (idx << 4 | total) & 0xFF, pad >> 8, pad & 0xFF])


@functools.lru_cache(maxsize=None)
def peek_plaintexts():
    """[(label, plaintext or None, raw wire or None)]: the peek lattice before obfuscation."""
    items = []
    for L in (0, 1, 7, 8):   # no plaintext at all
        items.append(("wire %d" % L, None, bytes(range(0x81, 0x81 + L))))
    for L in (9, 10, 12, 13, 14):   # 1..6 plaintext bytes: the first byte decides
        for first in (0x00, 0x7F, 0x80, 0xFF):
            items.append(("wire %d first %02x" % (L, first), bytes([first]) + _fill(L, L - 9), None))
    # a whole header in 5 and 6 bytes: empty payload, one payload byte, truncated by one
    items += [("hdr pad0 len5", _hdr(0x80, 3, 1, 2, 0), None), ("hdr pad1 len5", _hdr(0x80, 3, 1, 2, 1), None),
              ("hdr pad0 len6", _hdr(0x80, 3, 0, 2, 0) + b"x", None), ("hdr pad1 len6", _hdr(0x80, 3, 0, 2, 1) + b"p", None),
              ("hdr pad2 len6", _hdr(0x80, 3, 0, 2, 2) + b"p", None)]
    k = 0
    for total in (0, 1, 2, 8, 9, 15):
        for idx in sorted({0, max(total - 1, 0), total, 15}):
            for pad in (0, 1, 65535):
                for what, ln in (("empty", 5 + pad), ("truncated", 5 + pad - 1), ("data", 5 + pad + 3)):
                    for flag in (0x80, 0xC1):
                        if flag == 0xC1 and (pad == 65535 or what == "data"):
                            continue   # the flag's other bits: on the small ones only
                        k += 1
                        body = (_hdr(flag, k, idx, total, pad) + _fill(k, max(ln - 5, 0)))[:ln]
                        items.append(("t%d i%d pad%d %s flag%02x" % (total, idx, pad, what, flag), body, None))
    for j in range(40):   # top bit clear over an otherwise valid header, and plain garbage
        body = _fill(500 + j, 1 + (7 * j) % 60)
        if j % 2:
            body = _hdr(0x7F, j, 0, 2, 0) + body
        items.append(("pass %d" % j, body, None))
    # spread the 64 KiB ones: every prefix of the lattice holds some
    order = sorted(range(len(items)), key=lambda i: sref.splitmix64_at(3, i))
    return tuple(items[i] for i in order)


def peek_wires(psk: bytes, small: bool = False):
    out = []
    for i, (label, plain, raw) in enumerate(peek_plaintexts()):
        if small and plain is not None and len(plain) > 200:
            continue
        out.append((label, raw if plain is None else sref.obfuscate(psk, plain, _salt(i))))
    return out


def peek_case(name, psk, wires, layout):
    lens = [len(w) for _, w in wires]
    off, total = layout(lens)
    return {"name": name, "psk": psk, "labels": [l for l, _ in wires], "wires": [w for _, w in wires], "off": off,
            "len": np.array(lens, np.uint32), "buf_len": total}


@functools.lru_cache(maxsize=None)
def peek_cases():
    whole = peek_wires(PSK)
    cases = [peek_case("whole packed", PSK, whole, packed), peek_case("whole slotted", PSK, whole, slotted)]
    cases += [peek_case("first %d" % n, PSK, whole[:n], packed) for n in PEEK_NS]
    for pl in PSK_LENS:
        cases.append(peek_case("psk %d" % pl, psk_of(pl), peek_wires(psk_of(pl), small=True)[:65], slotted))
    return cases


def expected_peek(case):
    """(records, keys): keys[i] stays GUARD for a datagram of at most eight bytes."""
    n = len(case["wires"])
    recs = np.zeros(n, PARSED_DTYPE)
    keys = np.full((n, 32), GUARD, np.uint8)
    for i, w in enumerate(case["wires"]):
        recs[i] = record(case["psk"], w)
        if len(w) > 8:
            keys[i] = np.frombuffer(sref.key(case["psk"], w[:8]), np.uint8)
    return recs, keys


def blob_peek(case) -> bytes:
    n = len(case["wires"])
    return (struct.pack("<II", 1, len(case["psk"])) + case["psk"] + struct.pack("<QI", case["buf_len"], n) +
            case["off"].astype("<u8").tobytes() + case["len"].astype("<u4").tobytes() + b"".join(case["wires"]))


# ------------------------------------------------------------------ open
class Table:
    """Slots of one wire buffer, each with the record and key peek would leave."""

    def __init__(self):
        self.wires, self.off, self.recs, self.keys, self.wlen, self.payloads = [], [], [], [], [], []
        self.end = 0

    def _place(self, wire, residue):
        if residue is None:   # 8-aligned, at least one byte after the previous datagram
            off = (self.end + 8) // 8 * 8 if self.wires else 0
        else:
            off = self.end + (residue - self.end) % 16
        self.off.append(off)
        self.wires.append(wire)
        self.wlen.append(len(wire))
        self.end = off + len(wire)
        return len(self.wires) - 1

    def fragment(self, payload: bytes, pad: int, idx: int, total: int, msg_id: int = 1, residue=None) -> int:
        i = len(self.wires)
        plain = gref.encode_frame(gref.Header(pad, msg_id, idx, total), payload, _fill(2000 + i, pad))
        self.recs.append((FRAGMENT, pad, msg_id & 0xFF, idx << 4 | total, 5 + pad, len(payload)))
        self.keys.append(sref.key(PSK, _salt(i)))
        self.payloads.append(payload)
        return self._place(sref.obfuscate(PSK, plain, _salt(i)), residue)

    def passed(self, payload: bytes, residue=None) -> int:
        i = len(self.wires)
        payload = bytes([payload[0] & 0x7F]) + payload[1:]
        self.recs.append((PASS, 0, 0, 0, 0, len(payload)))
        self.keys.append(sref.key(PSK, _salt(i)))
        self.payloads.append(payload)
        return self._place(sref.obfuscate(PSK, payload, _salt(i)), residue)

    def forge(self, i: int, **fields) -> int:
        """A copy of slot i's datagram in a slot of its own with some record fields (or wire_len) changed."""
        j = self._place(self.wires[i], None)
        rec = dict(zip(PARSED_DTYPE.names, self.recs[i]))
        self.wlen[j] = fields.pop("wire_len", self.wlen[i])
        rec.update(fields)
        self.recs.append(tuple(rec[f] for f in PARSED_DTYPE.names))
        self.keys.append(self.keys[i])
        self.payloads.append(None)
        return j


def open_case(name, tab: Table, lists, caps, gaps):
    first = np.zeros(len(lists) + 1, np.uint64)
    np.cumsum([len(l) for l in lists], out=first[1:])
    out_off, at = [], 0
    for c, g in zip(caps, gaps):
        at += g
        out_off.append(at)
        at += c
    return {"name": name, "wires": tab.wires, "off": np.array(tab.off, np.uint64), "len": np.array(tab.wlen, np.uint32),
            "buf_len": tab.end, "recs": np.array(tab.recs, PARSED_DTYPE), "payloads": tab.payloads,
            "keys": np.frombuffer(b"".join(tab.keys), np.uint8).reshape(-1, 32), "lists": lists,
            "idx": np.array([i for l in lists for i in l], np.uint32), "first": first, "caps": np.array(caps, np.uint32),
            "gaps": np.array(gaps, np.uint32), "out_off": np.array(out_off, np.uint64), "out_total": at + OUT_TAIL}


def _pool_message(tab: Table, j: int):
    """Message j of the pool: its list and its payload.  Totals 2..8 with the lengths of
    OPEN_LENS in rotation, every ninth a single PASS slot; odd ones are put into the table
    in reversed slot order, every fifth with unrelated datagrams between its chunks; every
    fourteenth (one of five chunks) names its first slot twice."""
    if j % 9 == 8:
        ln = OPEN_LENS[1 + (j // 9) % (len(OPEN_LENS) - 1)]
        s = tab.passed(_fill(j, ln))
        return [s], tab.payloads[s]
    total = 2 + j % 7
    lens = [OPEN_LENS[(j // 7 + 3 * k) % len(OPEN_LENS)] for k in range(total)]
    pads = [(j + 5 * k) % 32 + (27 if (j + k) % 11 == 0 else 0) for k in range(total)]
    chunks = [_fill(j * 16 + k, lens[k]) for k in range(total)]
    slots = [None] * total
    for k in (reversed(range(total)) if j % 2 else range(total)):
        slots[k] = tab.fragment(chunks[k], pads[k], k, total, msg_id=j)
        if j % 5 == 0:
            tab.passed(_fill(900 + j, 1200))
    if j % 14 == 3:   # five chunks: a list of six
        return [slots[0]] + slots, chunks[0] + b"".join(chunks)
    return slots, b"".join(chunks)


def pool_case(m: int):
    tab, lists, want = Table(), [], []
    for j in range(m):
        l, d = _pool_message(tab, j)
        lists.append(l)
        want.append(d)
    caps = [len(d) - (1 if j % 4 == 3 and d else 0) for j, d in enumerate(want)]   # exact, or one short: ERR_CAP
    gaps = [1 + (5 * j) % 22 for j in range(m)]
    return dict(open_case("pool m=%d" % m, tab, lists, caps, gaps), want=want)


@functools.lru_cache(maxsize=None)
def residue_case():
    """(wire_off + 8 + payload_off) mod 16 x out_off mod 16 x payload_off mod 32, crossed:
    per output residue 64 messages of 8 pieces, which between them have every pair of the
    other two."""
    tab, lists, want, gaps, at = Table(), [], [], [], 0
    for r_o in range(16):
        for g in range(64):
            slots, data = [], b""
            for k in range(8):
                c = g * 8 + k
                src_res, po = c % 16, c // 16 if c // 16 >= 5 else c // 16 + 32
                payload = _fill(c + 512 * r_o, 17 + c % 7)
                slots.append(tab.fragment(payload, po - 5, k, 8, msg_id=g, residue=(src_res - 8 - po) % 16))
                data += payload
            lists.append(slots)
            want.append(data)
            gap = (r_o - at) % 16 or 16
            gaps.append(gap)
            at += gap + len(data)
    return dict(open_case("residues", tab, lists, [len(d) for d in want], gaps), want=want)


@functools.lru_cache(maxsize=None)
def plan_case():
    """Every ERR_PLAN cause, one at a time, between messages that open."""
    tab = Table()
    a = [tab.fragment(_fill(k, 40 + k), k, k, 2, msg_id=9) for k in range(2)]
    p = tab.passed(_fill(5, 33))
    nine = [tab.fragment(_fill(20 + k, 9), 0, k % 8, 8, msg_id=8) for k in range(9)]
    good = (a, tab.payloads[a[0]] + tab.payloads[a[1]])
    n_before = len(tab.wires)
    bad = [("empty list", []), ("nine entries", nine), ("index == n", [a[0], -1]), ("index 2^32 - 1", [0xFFFFFFFF, a[1]]),
           ("PASS in a list of two", [a[0], p]), ("two PASS slots", [p, p])]
    for st in (EMPTY, TRUNCATED, INVALID, 2, -1):
        bad.append(("status %d" % st, [a[0], tab.forge(a[1], status=st)]))
    bad += [("payload_len + 1", [tab.forge(a[0], payload_len=41), a[1]]),
            ("payload_len - 1", [tab.forge(a[0], payload_len=39), a[1]]),
            ("payload_off + 1", [a[0], tab.forge(a[1], payload_off=7)]),
            ("wire_len + 1", [tab.forge(a[0], wire_len=8 + 5 + 40 + 1), a[1]]),
            ("wire_len 4", [tab.forge(p, wire_len=4, payload_len=0)]),
            ("payload_len wraps 32 bits", [tab.forge(a[0], payload_off=5, payload_len=0xFFFFFFFF, wire_len=12), a[1]])]
    n = len(tab.wires)
    lists, want, exp = [], [], []
    for label, l in bad:
        lists += [good[0], [n if i == -1 else i for i in l]]
        want += [good[1], b""]
        exp += [OK, ERR_PLAN]
    lists += [[p], nine[:8]]
    want += [tab.payloads[p], b"".join(tab.payloads[i] for i in nine[:8])]
    exp += [OK, OK]
    assert n > n_before
    m = len(lists)
    return dict(open_case("plan errors", tab, lists, [max(len(d), 64) + 2 for d in want], [1 + (3 * j) % 19 for j in range(m)]),
                want=want, exp=exp, labels=[l for l, _ in bad])


def open_cases():
    return [pool_case(m) for m in OPEN_MS] + [residue_case(), plan_case()]


def expected_open(case):
    """(status, out_len, out): the header's rules over the case's own arrays."""
    n, recs, wlen = len(case["wires"]), case["recs"], case["len"]
    status, out_len = [], []
    out = np.full(case["out_total"], GUARD, np.uint8)
    buf = wire_buffer(case)
    for j, l in enumerate(case["lists"]):
        ok = 0 < len(l) <= 8 and all(i < n for i in l)
        ok = ok and all(recs[i]["status"] in (PASS, FRAGMENT) for i in l)
        ok = ok and not (len(l) > 1 and any(recs[i]["status"] == PASS for i in l))
        ok = ok and all(int(recs[i]["payload_off"]) + int(recs[i]["payload_len"]) == int(wlen[i]) - 8 for i in l)
        total = sum(int(recs[i]["payload_len"]) for i in l) if ok else 0
        st = ERR_PLAN if not ok else ERR_CAP if total > int(case["caps"][j]) else OK
        status.append(st)
        out_len.append(total if st == OK else 0)
        if st != OK:
            continue
        at = int(case["out_off"][j])
        for i in l:
            po, pl = int(recs[i]["payload_off"]), int(recs[i]["payload_len"])
            src = int(case["off"][i]) + 8 + po
            ks = np.resize(np.roll(case["keys"][i], -(po % 32)), pl)   # the key phase is the plaintext index
            out[at:at + pl] = buf[src:src + pl] ^ ks
            at += pl
    return np.array(status, np.int32), np.array(out_len, np.uint32), out


def blob_open(case) -> bytes:
    n, m = len(case["wires"]), len(case["lists"])
    real = np.array([len(w) for w in case["wires"]], np.uint32)
    return (struct.pack("<IQIII", 2, case["buf_len"], n, len(case["idx"]), m) + case["off"].astype("<u8").tobytes() +
            case["len"].astype("<u4").tobytes() + real.tobytes() + case["recs"].tobytes() + case["keys"].tobytes() +
            case["idx"].astype("<u4").tobytes() + case["first"].astype("<u8").tobytes() +
            case["caps"].astype("<u4").tobytes() + case["gaps"].astype("<u4").tobytes() + b"".join(case["wires"]))


# ------------------------------------------------------------------ checks, shared by both tiers
def check_peek(case, recs, keys):
    """All 16 bytes of every record, every key, and the key ranges that must stay untouched."""
    e_recs, e_keys = expected_peek(case)
    got = np.frombuffer(bytes(recs), PARSED_DTYPE)
    bad = [i for i in range(len(e_recs)) if got[i].tobytes() != e_recs[i].tobytes()]
    assert not bad, (case["name"], [(case["labels"][i], got[i], e_recs[i]) for i in bad[:4]])
    k = np.frombuffer(bytes(keys), np.uint8).reshape(-1, 32)
    bad = [i for i in range(len(e_recs)) if not np.array_equal(k[i], e_keys[i])]
    assert not bad, (case["name"], [case["labels"][i] for i in bad[:4]])


def check_open(case, status, out_len, out):
    e_status, e_len, e_out = expected_open(case)
    name = case["name"]
    assert list(status) == list(e_status), (name, [j for j, (a, b) in enumerate(zip(status, e_status)) if a != b][:8])
    assert list(out_len) == list(e_len), (name, [j for j, (a, b) in enumerate(zip(out_len, e_len)) if a != b][:8])
    got = np.frombuffer(bytes(out), np.uint8)
    assert len(got) == len(e_out), name
    if not np.array_equal(got, e_out):   # guard bytes included
        at = int(np.flatnonzero(got != e_out)[0])
        j = int(np.searchsorted(case["out_off"], at, side="right")) - 1
        raise AssertionError((name, "first differing output byte", at, "message", j, "of", int((got != e_out).sum())))
