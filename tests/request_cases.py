"""The lattices of the request hook (include/hyobfs_request.h), shared by the CPU tier
(tests/test_request.py: the scalar ABI and the emulated kernels) and the GPU tier
(tests/test_gpu_request.py): the items, their layout in poisoned buffers, the files
the stand-alone driver (tests/emu/request_main.cpp) reads and writes, and the checks
against the restatement (tests/request_ref.py).  TEST INFRASTRUCTURE ONLY."""
import functools
import random
import struct

import numpy as np

import addr_cases as ac
import addr_ref as A
import request_ref as R

GUARD, GUARD_BYTES = ac.GUARD, ac.GUARD_BYTES
NS = (0, 1, 63, 64, 65, 129)   # wave boundaries fall inside a batch
POISON = b":][@%+-0189\xff\x40\x80"
SRES_DTYPE = np.dtype([("status", "<i4"), ("name_len", "<u4"), ("name_off", "<u4"), ("need", "<u4")])
RANGE_DTYPE = np.dtype([("start", "<u2"), ("end", "<u2")])
BASE_OFF = 0x2_0000_0100
SEED = 0x5EED_0F_9ADD1
V6_45 = b"0000:0000:0000:0000:0000:ffff:255.255.255.255"   # the longest literal
assert len(V6_45) == A.LITERAL_MAX and A.parse_ip(V6_45) is not None


def layout(items, mod=16, skip=()) -> tuple[bytes, list[int], list[int]]:
    """(src, off, len): gaps of poison bytes between the items, so that item k starts at an offset that is
    k mod ``mod``.  The items whose index is in ``skip`` get no bytes at all: their offset points into poison."""
    rng = random.Random(len(items))
    buf, off = bytearray(), []
    for k, t in enumerate(items):
        gap = 1 + (k - len(buf) - 1) % mod
        buf += bytes(rng.choice(POISON) for _ in range(gap))
        off.append(len(buf))
        if k not in skip:
            buf += t
    buf += bytes(rng.choice(POISON) for _ in range(9))
    return bytes(buf), off, [len(t) for t in items]


def _batches(name, items, seed, **kw):
    """The whole lattice as one batch, and batches of every size of NS drawn from it."""
    rng = random.Random(seed)
    return [dict(name=name, items=list(items), **kw)] + [
        dict(name=f"{name}_n{n}", items=[rng.choice(items) for _ in range(n)], **kw) for n in NS]


# ------------------------------------------------------------------ request parse
def request(addr: bytes, pad: int = 0, rest: bytes = b"", addr_form: int = 0, pad_form: int = 0, addr_len=None) -> bytes:
    """A stream prefix behind the frame type; the padding and the rest are poison for a parser that strays."""
    n = len(addr) if addr_len is None else addr_len
    return R.varint(n, addr_form) + addr + R.varint(pad, pad_form) + b"\xff" * pad + rest


@functools.lru_cache(maxsize=None)
def parse_items() -> tuple:
    host = lambda n: ac._host(n - 3) + b":80" if n > 3 else b"a:1"[:n]   # noqa: E731
    out = []
    for n in (1, 63, 64, 2048):                                   # the address length in its minimal form
        out.append(request(host(n), 2, b"GET"))
    out.append(request(host(2049), 0, b"GET"))                       # ADDR_LEN
    out.append(request(b"", 0, b"GET"))                              # ADDR_LEN: 0
    for form in (2, 4, 8):                                          # 14 in each non-minimal form
        out.append(request(b"example.org:80", 3, b"\x16\x03\x01", addr_form=form, pad_form=form))
    out.append(R.varint((1 << 32) + 14, 8) + b"example.org:80" + b"\x00")   # must not wrap to 14
    for form in (2, 4, 8):
        out.append(R.varint(0, form) + b"x")                         # 0 in a long form
    small = request(b"example.org:80", 5, b"abc", addr_form=2, pad_form=2)
    out += [small[:k] for k in range(len(small) + 1)]                # cut at every prefix length
    bad_pad = R.varint(3) + b"a:1" + R.varint(4097, 4) + b"\xff" * 9
    out += [bad_pad[:k] for k in range(len(bad_pad) + 1)]            # PADDING_LEN as soon as the varint is whole
    bad_addr = R.varint(2049, 4) + b"a:1"
    out += [bad_addr[:k] for k in range(len(bad_addr) + 1)]          # ADDR_LEN as soon as the varint is whole
    for pad in (0, 1, 4096, 4097):
        for rest in (0, 1, 300):
            out.append(request(b"[2001:db8::1]:443", pad, b"\x16" * rest))
    out.append(request(b"a:1", 4096)[:-1])                            # one byte short of the padding
    return tuple(out)


def parse_cases() -> list[dict]:
    return _batches("parse", parse_items(), 0x9A85E)


PARSE_OUT = (("status", np.int32), ("need", np.uint32), ("addr_off", np.uint64), ("addr_len", np.uint32),
             ("rest_off", np.uint64), ("rest_len", np.uint32))


def expected_parse(items, offs) -> list[tuple]:
    out = []
    for t, o in zip(items, offs):
        st, need, ao, al, used = R.read_tcp_request(t)
        out.append((st, need, o + ao, al, o + used, len(t) - used) if st == R.OK else (st, need, 0, 0, 0, 0))
    return out


def check_parse(name, items, offs, got: dict) -> None:
    for i, e in enumerate(expected_parse(items, offs)):
        g = tuple(int(got[k][i]) for k, _ in PARSE_OUT)
        assert g == e, (name, i, items[i][:40], g, e)


# ------------------------------------------------------------------ check
PORTS = [b"", b"+", b"-", b"+80", b"-1", b"-0", b"65535", b"65536", b"65616", b"0080", b"8_0", b" 80", b"80 ", b"0x50",
         b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"9" * 20,
         b"0" * 70 + b"80", b"80", b"0", b"+0", b"--1", b"+-1", b"1+", b"-65456", b"00000000000000000000065616",
         b"-" + b"0" * 30 + b"9223372036854775808", b"18446744073709551696"]
HOSTS = [b"1.2.3.4", b"[::1]", b"[::ffff:1.2.3.4]", b"example.com", b"", b"[" + V6_45 + b"5]", b"[" + V6_45 + b"]",
         b"1.2.3.04", b"[fe80::1%eth0]", b"[]"]
UNIONS = [None, [], [(0, 0)], [(80, 80)], [(65535, 65535)], [(90, 100), (70, 85), (80, 95), (443, 443)]]


@functools.lru_cache(maxsize=None)
def check_items() -> tuple:
    out = [b"@1.2.3.4:80", b"@"] + list(ac.H_CORPUS)
    out += [h + b":" + p for h in HOSTS for p in PORTS]
    for n in (63, 64, 65, 127, 128, 129, 2048, 2049):              # text lengths
        out.append(ac._host(n - 3) + b":80")
        out.append(b"1.2.3.4:" + b"0" * (n - 10) + b"80")
    # the digits, a sign or the last ':' on a window edge
    for zeros in (54, 55, 56, 118, 119, 120):
        out.append(b"1.2.3.4:" + b"0" * zeros + b"80")               # "80" straddles with 55 and 119 zeros
    out.append(ac._host(56) + b":" + b"0" * 70 + b"80")
    for n in (61, 62, 63, 64, 125, 126, 127, 128):                 # the ':' at index n
        for p in (b"+80", b"80", b"-1", b"+", b"x80", b"8x"):
            out.append(ac._host(n) + b":" + p)
    out.append(ac._host(50) + b":9223372036854775807")              # 19 digits over two windows
    out.append(ac._host(50) + b":9223372036854775808")
    out.append(b"[" + V6_45 + b"]:9223372036854775807")
    out.append(b"[" + V6_45 + b"]:-9223372036854775808")
    out.append(b"[" + V6_45 + b"]:-9223372036854775809")
    rng = random.Random(0xC4EC)
    alphabet = b"0123456789+-:.[]@%a_ "
    for _ in range(120):
        base = bytearray(rng.choice((b"1.2.3.4:80", b"[::1]:+443", b"a.b:-1", b"10.0.0.1:00000065616")))
        for _ in range(rng.randint(1, 3)):
            pos = rng.randrange(len(base) + 1)
            if rng.random() < 0.5:
                base.insert(pos, rng.choice(alphabet))
            elif base:
                base[min(pos, len(base) - 1)] = rng.choice(alphabet)
        out.append(bytes(base))
    return tuple(out)


def check_cases() -> list[dict]:
    items = check_items()
    cases = []
    k = 0
    for rd in (False, True):
        for is_udp in (False, True):
            u = UNIONS[(k * 2) % len(UNIONS)], UNIONS[(k * 2 + 1) % len(UNIONS)]
            cases.append(dict(name=f"check_rd{int(rd)}_udp{int(is_udp)}_a", items=list(items), rewrite_domain=rd,
                              is_udp=is_udp, union=u[0], gate=False))
            cases.append(dict(name=f"check_rd{int(rd)}_udp{int(is_udp)}_b", items=list(items[::3]), rewrite_domain=rd,
                              is_udp=is_udp, union=u[1], gate=bool(k % 2)))
            k += 1
    rng = random.Random(0xC4EC5)
    for j, n in enumerate(NS):
        cases.append(dict(name=f"check_n{n}", items=[rng.choice(items) for _ in range(n)], rewrite_domain=bool(j % 2),
                          is_udp=bool(j % 3 == 0), union=UNIONS[(j + 3) % len(UNIONS)], gate=bool(j % 2 == 0)))
    return cases


def gates(case) -> list[int]:
    """The gate of a case: every third item is closed (and has no bytes in the buffer)."""
    return [(-86 if k % 3 == 1 else 0) if case["gate"] else 0 for k in range(len(case["items"]))]


def closed(case) -> tuple:
    return tuple(k for k, g in enumerate(gates(case)) if g)


def expected_check(case) -> list[int]:
    g = gates(case)
    u = case["union"]
    return [0 if g[k] else int(R.check(t, case["is_udp"], case["rewrite_domain"], u, u))
            for k, t in enumerate(case["items"])]


def verify_check(case, got) -> None:
    exp = expected_check(case)
    assert len(got) == len(exp)
    for i, e in enumerate(exp):
        assert int(got[i]) == e, (case["name"], i, case["items"][i][:90], int(got[i]), e)


# ------------------------------------------------------------------ rewrite
NAME_STRIDE = 255
OK_, NEED_MORE_, HOST_, NAME_CAP_ = 0, R.SNIFF_NEED_MORE, R.SNIFF_HOST, R.SNIFF_NAME_CAP
OTHER_SNIFF = (-55, -65, -67)   # MALFORMED, NOT_HTTP, UNRECOGNIZED: the address stays


@functools.lru_cache(maxsize=None)
def rewrite_items() -> tuple:
    """(address, check, name, name_len reported, sniffer status)."""
    names = [b"a", bytes(97 + i % 26 for i in range(255)), b"fe80::1", b"a%b", "政府.中国".encode() + b"\x80\xff", b"example.org"]
    addrs = [b"1.2.3.4:80", b"[::1]:443", b"h:+80", b"10.0.0.1:" + b"0" * 300 + b"80", ac._host(60) + b":8", b"a:",
             ac._host(61) + b":80", ac._host(62) + b":80"]
    out = []
    for a in addrs:
        for chk in (0, 1):
            for nm in names:
                out.append((a, chk, nm, len(nm), OK_))
            out.append((a, chk, b"", 0, OK_))                        # a hello without a name
            out.append((a, chk, b"", 0, NEED_MORE_))
            out.append((a, chk, b"", 0, HOST_))
            out.append((a, chk, b"", 300, NAME_CAP_))                # the name did not fit its row: nothing is there
            for st in OTHER_SNIFF:
                out.append((a, chk, b"", 0, st))
    out.append((b"no-port", 1, b"x.org", 5, OK_))                    # MISSING_PORT
    out.append((b"no-port", 0, b"x.org", 5, OK_))
    out.append((b"", 0, b"", 0, OK_))
    return tuple(out)


def rewrite_one(item, gate=0):
    a, chk, nm, nlen, sst = item
    return R.rewrite(a, bool(chk), nm if sst == OK_ else b"", sst, gate)


def rewrite_cases() -> list[dict]:
    items = rewrite_items()
    fit = max(len(rewrite_one(x)[1]) for x in items)
    kw = dict(gate=False, mis=0)
    cases = [dict(name="rewrite_fit", items=list(items), stride=fit, **kw),
             dict(name="rewrite_fit_less_1", items=list(items), stride=fit - 1, gate=True, mis=1),
             dict(name="rewrite_small_odd", items=list(items[::2]), stride=21, gate=False, mis=3),
             dict(name="rewrite_wide", items=list(items[::5]), stride=fit + 37, gate=True, mis=2)]
    rng = random.Random(0x4E4)
    small = [x for x in items if len(x[0]) < 100]
    for j, n in enumerate(NS):
        cases.append(dict(name=f"rewrite_n{n}", items=[rng.choice(small) for _ in range(n)], stride=(263, 64, 275, 11)[j % 4],
                          gate=bool(j % 2), mis=j % 4))
    return cases


def rewrite_inputs(case):
    """(src, off, len, gate, check, sres records, names rows) of a case.  A names row holds its name and poison
    behind it; a row that must not be read is all poison."""
    items, g = case["items"], gates(case)
    src, off, lens = layout([x[0] for x in items], skip=closed(case))
    sres = np.zeros(len(items), SRES_DTYPE)
    names = np.full((len(items), NAME_STRIDE), ord(":"), np.uint8)
    for k, (a, chk, nm, nlen, sst) in enumerate(items):
        sres[k] = (sst, nlen, 5 if nlen else 0, 7 if sst == NEED_MORE_ else 0)
        names[k, :len(nm)] = np.frombuffer(nm, np.uint8)
    return src, off, lens, g, [x[1] for x in items], sres, names.reshape(-1)


def name_reads(case) -> list[int]:
    """How many bytes of each names row the call may read."""
    g = gates(case)
    return [nlen if (not g[k] and chk and sst == OK_) else 0 for k, (a, chk, nm, nlen, sst) in enumerate(case["items"])]


def verify_rewrite(case, status, out_len, rewritten, row_off, out, base_off=BASE_OFF) -> None:
    """``out``: the n * stride bytes, pre-filled with GUARD."""
    n, stride, g = len(case["items"]), case["stride"], gates(case)
    assert len(out) == n * stride
    for i, item in enumerate(case["items"]):
        st, text, rew = rewrite_one(item, g[i])
        row = bytes(out[i * stride:(i + 1) * stride])
        assert int(row_off[i]) == base_off + i * stride, (case["name"], i)
        if st == R.OK and len(text) > stride:
            e = (R.CAP, len(text), 0, bytes([GUARD]) * stride)          # nothing of the row is written
        elif st == R.OK:
            e = (R.OK, len(text), rew, text + bytes(stride - len(text)))
        else:
            e = (st, 0, 0, bytes(stride))
        assert (int(status[i]), int(out_len[i]), int(rewritten[i]), row) == e, (case["name"], i, item[:2], item[3:], e[:3])


# ------------------------------------------------------------------ response build
MSGS = [b"", b"C", b"RequestHook enabled".ljust(63, b"!"), b"x" * 64, bytes(33 + i % 90 for i in range(2048)), b"Connected"]
PADS = (0, 1, 63, 64, 127, 128, 1023, 4096)


@functools.lru_cache(maxsize=None)
def response_items() -> tuple:
    """(ok, msg_idx, pad_len)."""
    out = [((m + p) % 2, m, p) for m in range(len(MSGS)) for p in PADS]
    out.append((1, len(MSGS), 5))           # no such message
    out.append((0, 0xFFFFFFFF, 0))
    out += [(1, 5, p) for p in (2, 3, 4, 5, 6, 7, 8, 9)]   # the padding starts at every phase of a dword
    return tuple(out)


def response_one(item, i, seed=SEED):
    ok, m, p = item
    return None if m >= len(MSGS) else R.write_tcp_response(bool(ok), MSGS[m], p, seed, i)


def response_cases() -> list[dict]:
    items = response_items()
    fit = max(len(response_one(x, 0)) for x in items if x[1] < len(MSGS))
    assert fit == 1 + 2 + 2048 + 2 + 4096
    cases = [dict(name="response_fit", items=list(items), stride=fit, mis=0),
             dict(name="response_fit_less_1", items=list(items), stride=fit - 1, mis=1),
             dict(name="response_odd", items=list(items), stride=1041, mis=3)]
    rng = random.Random(0x4E5)
    small = [x for x in items if x[1] != 4 and x[2] <= 1023]
    for j, n in enumerate(NS):
        cases.append(dict(name=f"response_n{n}", items=[rng.choice(small) for _ in range(n)], stride=(1100, 131, 1097, 64)[j % 4],
                          mis=j % 4))
    return cases


def response_inputs(case):
    """(ok u8, msg_idx u32, pad_len u32, msgs buffer, msg_off u64, msg_len u32)."""
    buf, off, lens = layout(MSGS, mod=4)
    it = case["items"]
    return (np.array([x[0] for x in it], np.uint8), np.array([x[1] for x in it], np.uint32),
            np.array([x[2] for x in it], np.uint32), buf, np.array(off, np.uint64), np.array(lens, np.uint32))


def verify_response(case, status, out_len, out, parse_back=None, seed=SEED) -> None:
    """``out``: the n * stride bytes, pre-filled with GUARD: exactly [0, out_len) of a row is written.
    ``parse_back(frame)``: the library's response parser, (status, need, ok, msg_off, msg_len, consumed)."""
    n, stride = len(case["items"]), case["stride"]
    assert len(out) == n * stride
    for i, item in enumerate(case["items"]):
        e = response_one(item, i, seed)
        row = bytes(out[i * stride:(i + 1) * stride])
        if e is None:
            want = (-2, 0, bytes([GUARD]) * stride)
        elif len(e) > stride:
            want = (R.CAP, len(e), bytes([GUARD]) * stride)
        else:
            want = (R.OK, len(e), e + bytes([GUARD]) * (stride - len(e)))
            pad = e[len(e) - item[2]:] if item[2] else b""
            assert pad == R.padding(seed, i, item[2]) and all(c in R.PADDING_CHARS for c in pad)
        assert (int(status[i]), int(out_len[i]), row) == want, (case["name"], i, item, int(status[i]), int(out_len[i]))
        if parse_back is not None and want[0] == R.OK:
            m = MSGS[item[1]]
            off = 1 + len(R.varint(len(m)))
            assert parse_back(e) == (R.OK, 0, int(bool(item[0])), off, len(m), len(e)), (case["name"], i)


# ------------------------------------------------------------------ port unions
UNION_TEXTS = [b"", b",", b"1-2-3", b"5-1", b"65535-65535", b"0-65535,1", b"1-2,3-4", b"1-2,4-5", b"all", b"*", b"all,1", b"80",
               b"080", b"65536", b"-1", b"1-", b"+1", b"1 ", b"1,,2", b"3-4,1-2", b"10-20,15-30,31-40,42", b"0,65535,65534",
               b"0-0", b"1_0", b"0x10", b"443,80,443"]


# ------------------------------------------------------------------ the emulated driver's files
def _arrays(off, lens):
    return np.array(off, "<u8").tobytes() + np.array(lens, "<u4").tobytes()


def blob_parse(case) -> bytes:
    buf, off, lens = layout(case["items"])
    return struct.pack("<III", 1, len(off), len(buf)) + buf + _arrays(off, lens)


def blob_check(case) -> bytes:
    buf, off, lens = layout(case["items"], skip=closed(case))
    u = case["union"]
    b = struct.pack("<IIIIIiI", 2, len(off), len(buf), int(case["is_udp"]), int(case["rewrite_domain"]),
                    -1 if u is None else len(u), int(case["gate"]))
    b += buf + _arrays(off, lens)
    if case["gate"]:
        b += np.array(gates(case), "<i4").tobytes()
    return b + np.array(u or [], "<u2").tobytes()


def blob_rewrite(case) -> bytes:
    src, off, lens, g, chk, sres, names = rewrite_inputs(case)
    b = struct.pack("<IIIIIIIQ", 3, len(off), len(src), NAME_STRIDE, case["stride"], case["mis"], int(case["gate"]), BASE_OFF)
    b += src + _arrays(off, lens)
    if case["gate"]:
        b += np.array(g, "<i4").tobytes()
    return (b + np.array(chk, np.uint8).tobytes() + sres.tobytes() + names.tobytes()
            + np.array(name_reads(case), "<u4").tobytes())


def blob_response(case) -> bytes:
    ok, idx, pad, mbuf, moff, mlen = response_inputs(case)
    b = struct.pack("<IIIIIQI", 4, len(ok), len(MSGS), case["stride"], case["mis"], SEED, len(mbuf))
    return b + mbuf + moff.astype("<u8").tobytes() + mlen.astype("<u4").tobytes() + ok.tobytes() + idx.tobytes() + pad.tobytes()


# ------------------------------------------------------------------ the golden file
def golden_lattice() -> dict:
    """A sample of the lattice's expected outputs from the restatement (tests/golden/request_vectors.json, "lattice"):
    every few items of each lattice, the short ones, so that the file stays readable."""
    hx = lambda b: bytes(b).hex()   # noqa: E731
    g = {"request": [], "response": [], "union": [], "check": [], "rewrite": [], "padding": []}
    for t in [t for t in parse_items() if len(t) <= 60][::3]:
        g["request"].append({"hex": hx(t), "result": list(R.read_tcp_request(t))})
    frames = [(i, x, response_one(x, i)) for i, x in enumerate(response_items()) if x[1] < len(MSGS)]
    for i, item, e in [f for f in frames if len(f[2]) <= 100][::3]:
        g["response"].append({"ok": item[0], "msg": hx(MSGS[item[1]]), "pad_len": item[2], "item": i, "hex": hx(e)})
        for cut in (1, len(e) // 2):
            g["response"].append({"parse": hx(e[:cut]), "result": list(R.read_tcp_response(e[:cut]))})
    for t in UNION_TEXTS:
        g["union"].append({"text": t.decode(), "ranges": R.parse_port_union(t)})
    for t in [t for t in check_items() if len(t) <= 60][::5]:
        g["check"].append({"hex": hx(t), "verdicts": [
            int(R.check(t, bool(k & 1), bool(k & 2), UNIONS[3], UNIONS[5])) for k in range(4)]})
    for item in [x for x in rewrite_items() if len(x[0]) <= 40 and len(x[2]) <= 40][::5]:
        st, text, rew = rewrite_one(item)
        g["rewrite"].append({"addr": hx(item[0]), "check": item[1], "name": hx(item[2]), "name_len": item[3],
                             "sniff_status": item[4], "status": st, "text": hx(text), "rewritten": rew})
    for seed, item, n in ((0, 0, 16), (SEED, 7, 40), ((1 << 64) - 1, (1 << 64) - 1, 9)):
        g["padding"].append({"seed": seed, "item": item, "text": R.padding(seed, item, n).decode()})
    return g
