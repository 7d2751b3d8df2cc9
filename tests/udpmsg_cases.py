"""Case families of the UDP relay message kernels, shared by the CPU tier
(tests/test_udpmsg.py: the kernels compiled for the host under AddressSanitizer)
and the GPU tier (tests/test_gpu_udpmsg.py).  Expected values come from
tests/udpmsg_ref.py alone.

A send case is a dict: name, msgs = [(session_id, packet_id, addr, data,
max_size)], out_cap / dgram_cap (None: exactly what the batch needs), out_mis
(the misalignment of the output buffer's first byte, 0..15); spread = 1 (CPU tier
only) lays every payload and address out in a slot of its own with poisoned gaps.
"""
from __future__ import annotations

import functools
import random
import struct

import numpy as np

import udpmsg_ref as R

ADDR_LENS = (1, 2, 11, 63, 64, 65, 255, 2048)
MAX_PAYLOADS = (1, 2, 15, 16, 17, 63, 64, 65, 1180)
GUARD = 0xA5


def _addr(n: int) -> bytes:
    return bytes((0x61 + (i * 7 + n) % 26) for i in range(n))


def _data(rng: random.Random, n: int) -> bytes:
    return rng.randbytes(n)


def header_size(addr_len: int) -> int:
    return 8 + R.varint_len(addr_len) + addr_len


def data_lens(mp: int) -> list[int]:
    return sorted({0, 1, mp - 1, mp, mp + 1, 2 * mp - 1, 2 * mp, 2 * mp + 1, 255 * mp, 255 * mp + 1})


def lattice_msgs() -> list[tuple]:
    """Address length x maxPayload x data length; max_size <= HeaderSize (NO_ROOM)
    included.  Sizes whose serialised length exceeds 4096 stay in as A1 cases."""
    rng = random.Random(0x0DB5)
    msgs = []
    for al in ADDR_LENS:
        addr, h = _addr(al), header_size(al)
        for mp in MAX_PAYLOADS:
            for dl in data_lens(mp):
                msgs.append((rng.getrandbits(32), rng.randrange(1, 65536), addr, _data(rng, dl), h + mp))
        for max_size in (h, h - 1, 0):   # maxPayload <= 0
            msgs.append((rng.getrandbits(32), rng.randrange(1, 65536), addr, _data(rng, 40), max_size))
    return msgs


def residues(msgs) -> tuple[set, set]:
    """(source offsets mod 16 of the data packed back to back, output offsets mod 16 of the datagrams)."""
    src, at = set(), 0
    for m in msgs:
        if m[3]:
            src.add(at % 16)
        at += len(m[3])
    _, _, _, dgrams = R.send_batch(msgs)
    return src, {off % 16 for off, _ in dgrams}


def lattice_cases() -> list[dict]:
    msgs = lattice_msgs()
    return [dict(name="lattice", msgs=msgs, out_cap=None, dgram_cap=None, out_mis=0),
            dict(name="lattice_mis5", msgs=msgs, out_cap=None, dgram_cap=None, out_mis=5)]


def capacity_msgs() -> list[tuple]:
    rng = random.Random(0xCA9)
    a = b"10.0.0.1:53"
    return [(1, 11, a, _data(rng, 1350), 1200), (2, 12, a, _data(rng, 64), 1200), (3, 13, a, _data(rng, 5000), 1200),
            (4, 14, a, _data(rng, 300), 100), (5, 15, a, _data(rng, 33), 20), (6, 16, a, _data(rng, 1), 1200),
            (7, 17, a, _data(rng, 2000), 1200), (8, 18, a, _data(rng, 700), 21), (9, 19, a, _data(rng, 640), 333),
            (10, 20, a, _data(rng, 17), 1200)]


def capacity_cases() -> list[dict]:
    """out_cap / dgram_cap exactly enough, one short, and cutting the first, a middle and the last message."""
    msgs = capacity_msgs()
    status, first, (nbytes, nd), _ = R.send_batch(msgs)
    assert R.TOO_LARGE in status and R.NO_ROOM in status and R.FRAG_COUNT in status
    per = [sum(len(d) for d in R.send(*m[:2], m[2], m[3], m[4])[1]) for m in msgs]
    through = np.cumsum(per)
    out = []
    for name, oc, dc in (("exact", nbytes, nd), ("bytes_one_short", nbytes - 1, nd), ("dgrams_one_short", nbytes, nd - 1),
                         ("cut_first", per[0] - 1, nd), ("cut_first_dgrams", nbytes, first[1] - 1),
                         ("cut_middle", int(through[4]) - 3, nd), ("cut_middle_dgrams", nbytes, first[5] - 1),
                         ("cut_last", int(through[-1]) - per[-1], nd), ("roomy", nbytes + 100, nd + 7),
                         ("sizing_run", 0, 0)):
        out.append(dict(name="capacity_" + name, msgs=msgs, out_cap=oc, dgram_cap=dc, out_mis=3))
    return out


SCAN_REACH = 256 * 256   # messages one pass of the tile-sum scan covers (udpmsg.hip: 256 tiles of 256)
SMALL_SCAN_REACH = 64 * 64   # the same in the CPU tier's second build (-DHY_UDP_TILE_MSGS=64 -DHY_UDP_SCAN_TILES=64)


def scan_msgs(n: int) -> list[tuple]:
    return [(i, 1 + i % 65535, b"a", bytes([(i + k) & 0xFF for k in range(1 + i % 3)]), 11 + i % 2) for i in range(n)]


def scan_cases(reach: int = SCAN_REACH) -> list[dict]:
    """n = 1, 255, 256, 257 and one batch just beyond a single scan pass's reach (the GPU tier runs it on the
    library as shipped; the CPU tier, where a workgroup costs 256 host threads, on a build whose tiles and scan
    passes are 64 wide)."""
    ns = [1, 255, 256, 257, reach + 1]
    if reach != SCAN_REACH:
        ns += [63, 64, 65, reach]
    return [dict(name=f"scan_{n}", msgs=scan_msgs(n), out_cap=None, dgram_cap=None, out_mis=n % 16) for n in ns]


def random_msgs(n: int = 3000, seed: int = 7) -> list[tuple]:
    """Bimodal 64 / 1350 data, addresses of 9-40 bytes, max_size 1000 / 1200 / 1400: all OK by construction."""
    rng = random.Random(seed)
    addrs = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789.:") for _ in range(rng.randrange(9, 41)))
             for _ in range(32)]
    return [(rng.getrandbits(32), rng.randrange(1, 65536), rng.choice(addrs), _data(rng, rng.choice((64, 1350))),
             rng.choice((1000, 1200, 1400))) for _ in range(n)]


def random_case(n: int = 3000) -> dict:
    return dict(name="random_round_trip", msgs=random_msgs(n), out_cap=None, dgram_cap=None, out_mis=9)


def expected_send(case: dict):
    """(status, first, totals, out bytes with GUARD where nothing is written, dgram (off, len) list,
    out_cap, dgram_cap)."""
    _, _, (nbytes, nd), _ = R.send_batch(case["msgs"])
    oc = nbytes if case["out_cap"] is None else case["out_cap"]
    dc = nd if case["dgram_cap"] is None else case["dgram_cap"]
    status, first, totals, dgrams = R.send_batch(case["msgs"], oc, dc)
    out = bytearray([GUARD]) * oc
    for off, d in dgrams:
        out[off:off + len(d)] = d
    # entry first[i] + k of the datagram arrays, for the datagrams of written messages only
    entries, at = {}, 0
    for i, st in enumerate(status):
        if st == R.OK:
            for k in range(first[i + 1] - first[i]):
                entries[first[i] + k] = (dgrams[at][0], len(dgrams[at][1]))
                at += 1
    return status, first, totals, bytes(out), entries, oc, dc


# ------------------------------------------------------------------ parse
GOLDEN_MALFORMED = [b"", bytes(4), bytes(12), bytes.fromhex("66ccffff1122334455"),
                    bytes.fromhex("66ccffff1122334490aabbccddeeff")]


def produced_datagrams(scan_reach: int = SCAN_REACH) -> list[bytes]:
    """Every datagram the send cases produce: lattice, capacity, scan edges and the random round trip."""
    out = []
    for msgs in (lattice_msgs(), capacity_msgs(), *[c["msgs"] for c in scan_cases(scan_reach)], random_msgs()):
        for m in msgs:
            out += R.send(*m)[1]
    return out


def _header_len(d: bytes) -> int:
    vl = 1 << (d[8] >> 6)
    return 8 + vl + (int.from_bytes(d[8:8 + vl], "big") & ((1 << (8 * vl - 2)) - 1))


def parse_class(x: bytes) -> tuple:
    """All that ParseUDPMessage's verdict on x depends on: its length and the bytes it has of
    the varint.  (The eight bytes in front are only copied out, and only when the verdict is OK.)"""
    return len(x), bytes(x[8:8 + (1 << (x[8] >> 6))]) if len(x) > 8 else b""


def truncation_coverage(prod, items) -> None:
    """Asserts what parse_datagrams() states about `items`."""
    have, classes = set(items), {parse_class(x) for x in items}
    done = set()
    for d in prod:
        h = _header_len(d)
        assert d in have and d[:h + 1] in have
        if parse_class(d[:h]) not in done:
            done.add(parse_class(d[:h]))
            assert all(parse_class(d[:k]) in classes for k in range(h + 1))


@functools.lru_cache(maxsize=None)
def parse_datagrams(scan_reach: int = SCAN_REACH) -> tuple:
    """Every datagram the send cases produce, truncated at every length from 0 to header + 1,
    with the truncations that the parser cannot tell apart taken once.  In full:
      * every produced datagram whole, and cut at header + 1 (the only cut that can parse,
        so its eight leading bytes matter: every datagram's own);
      * the cuts at 0 .. header, whose verdict depends on the length and the varint bytes
        alone (parse_class), from one datagram per distinct varint, i.e. address length;
    then the malformed goldens, non-minimal varints in all four widths, address lengths
    63 / 64 / 2048 / 2049 and 8-byte varints that only fit 64 bits.  truncation_coverage()
    asserts the first two points."""
    prod = produced_datagrams(scan_reach)
    out, seen = list(prod), set()
    for d in prod:
        h = _header_len(d)
        if len(d) > h + 1:
            out.append(d[:h + 1])
        varint = d[8:8 + (1 << (d[8] >> 6))]
        if varint not in seen:
            seen.add(varint)
            out += [d[:k] for k in range(h + 1)]
    out += GOLDEN_MALFORMED
    head = bytes.fromhex("0000002a00070102")
    for form in R.varint_forms(5):
        out += [head + form + b"addr:" + b"xy", head + form + b"addr:", head + form + b"addr", head + form[:-1]]
    for al in (63, 64, 2048, 2049):
        for form in R.varint_forms(al):
            out += [head + form + _addr(al) + b"d", head + form + _addr(al)]
    out.append(head + bytes.fromhex("c000000100000005") + b"addr:x")   # 2^32 + 5: huge as a 64-bit value
    out.append(head + bytes.fromhex("ffffffffffffffff") + b"addr:x")
    return tuple(out)


def pack(items) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    lens = np.array([len(p) for p in items], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if len(items) > 1:
        np.cumsum(lens[:-1], out=off[1:])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off, lens


# ------------------------------------------------------------------ defragment / assemble
def defrag_stream(seed: int = 3, sessions: int = 5, per_session: int = 6):
    """Datagrams of interleaved sessions in arrival order.  Within a session the
    messages follow one another with their fragments shuffled; some fragments
    arrive twice (D4), and after some completed messages one of their fragments
    arrives again (D6: swallowed)."""
    rng = random.Random(seed)
    queues = []
    for s in range(sessions):
        q = []
        for k in range(per_session):
            data = _data(rng, rng.choice((30, 64, 700, 1350, 2500)))
            st, ds = R.send(100 + s, 1 + 10 * s + k, b"host%d.example:443" % s, data, rng.choice((200, 600, 1200)))
            assert st == R.OK
            ds = list(ds)
            rng.shuffle(ds)
            if len(ds) > 1 and rng.random() < 0.5:
                ds.insert(rng.randrange(1, len(ds)), ds[0])      # a duplicate before completion
            if len(ds) > 1 and rng.random() < 0.5:
                ds.append(ds[rng.randrange(len(ds))])            # stale: after completion
            q += ds
        queues.append(q)
    stream = []
    while any(queues):
        q = rng.choice([q for q in queues if q])
        stream.append(q.pop(0))
    return stream


def expected_defrag(stream):
    """The reference's receive loop: per SessionID a Defragger; [(session_id, addr, data)] in completion order."""
    ds, out = {}, []
    for d in stream:
        m = R.parse(d)
        if not isinstance(m, R.UDPMessage):
            continue
        r = ds.setdefault(m.session_id, R.Defragger()).feed(m)
        if r is not None:
            out.append((r.session_id, r.addr, r.data))
    return out


def assemble_plan_cases(n: int, ok_idx: list[int], bad_idx: int):
    """Fragment lists with each ERR_PLAN cause, next to good ones: (lists, expected statuses or None for OK)."""
    lists = [[ok_idx[0]], [], [ok_idx[0], ok_idx[1]], [ok_idx[0]] * 256, [ok_idx[1]] * 255, [ok_idx[0], n],
             [0xFFFFFFFF], [ok_idx[1], bad_idx], [ok_idx[1]]]
    exp = [None, R.PLAN, None, R.PLAN, None, R.PLAN, R.PLAN, R.PLAN, None]
    return lists, exp


# ------------------------------------------------------------------ the CPU driver's file format (tests/emu/udpmsg_main.cpp)
def blob_send(case: dict) -> bytes:
    _, _, _, _, _, oc, dc = expected_send(case)
    msgs = case["msgs"]
    addrs, where = bytearray(), {}
    for m in msgs:
        if m[2] not in where:
            where[m[2]] = len(addrs)
            addrs += m[2]
    b = struct.pack("<IIQQII", 1, len(msgs), oc, dc, case["out_mis"], case.get("spread", 0))
    b += struct.pack("<I", len(addrs)) + bytes(addrs)
    for sid, pid, addr, data, max_size in msgs:
        b += struct.pack("<IIIIQI", sid, pid, max_size, len(addr), where[addr], len(data))
    return b + b"".join(m[3] for m in msgs)


def blob_parse(items) -> bytes:
    return struct.pack("<II", 2, len(items)) + b"".join(struct.pack("<I", len(d)) + d for d in items)


def blob_assemble(items, lists, caps, gaps) -> bytes:
    b = struct.pack("<II", 3, len(items)) + b"".join(struct.pack("<I", len(d)) + d for d in items)
    idx = [i for l in lists for i in l]
    b += struct.pack("<I", len(idx)) + struct.pack(f"<{len(idx)}I", *idx) + struct.pack("<I", len(lists))
    first = [0]
    for l in lists:
        first.append(first[-1] + len(l))
    b += struct.pack(f"<{len(first)}Q", *first)
    return b + b"".join(struct.pack("<II", c, g) for c, g in zip(caps, gaps))
