"""CPU tier of Gecko's device receive path (include/hyobfs_gecko.h): the C reassembler
against the restatement (tests/gecko_rx_ref.py) on random streams and on the
scenarios of the reference's gecko_test.go, and the peek and open kernels over the
lattices of tests/gecko_rx_cases.py through tests/emu/gecko_rx_main.cpp, a stand-alone
AddressSanitizer program linked against the emulated library and run as a child
process (nothing is preloaded)."""
import fcntl
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import gecko_rx_cases as gc
import gecko_rx_ref as R
from hysteria_amd import _lib, gecko
from hysteria_amd.gecko import GeckoReceiver, Reassembler, open_batch, peek_batch  # noqa: F401  (the feature under test)
from oracle import gecko_ref as gref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


# ------------------------------------------------------------------ the reassembler
def _rec(status, msg_id=0, idx=0, total=0, pad=0, payload_len=0) -> bytes:
    off = 5 + pad if status == gecko.FRAGMENT else 0
    return np.array([(status, pad, msg_id, (idx << 4 | total) & 0xFF, off, payload_len)], gecko.PARSED_DTYPE).tobytes()


_KIND = {gecko.PASS: gref.PASS, gecko.FRAGMENT: gref.FRAGMENT, gecko.EMPTY: gref.EMPTY,
         gecko.ERR_TRUNCATED: gref.TRUNCATED, gecko.ERR_INVALID: gref.INVALID}


class _Pair:
    """The C reassembler and the restatement, fed the same things; every answer compared."""

    def __init__(self):
        self.c, self.r, self.tag, self.codes = gecko.Reassembler(), R.Conn(), 0, {}

    def feed(self, source, status, msg_id=0, idx=0, total=0, payload_len=0, now=0):
        self.tag += 1
        got = self.c.feed(source, _rec(status, msg_id, idx, total, 0, payload_len), self.tag, now)
        want = self.r.feed(source, _KIND[status], msg_id, idx, total, payload_len, self.tag, now)
        assert got == want, (source, status, msg_id, idx, total, now)
        self.codes[got[0]] = self.codes.get(got[0], 0) + 1
        return got

    def gc(self, now):
        self.c.gc(now)
        self.r.gc_expired(now)

    def check(self):
        assert self.c.pending() == len(self.r.reassembly)
        rel = self.c.released()
        assert rel == self.r.take_released()
        return rel


@pytest.mark.parametrize("seed", [1, 2])
def test_reassembler_random_streams(seed):
    """At least 20 000 feeds (clock steps and gc calls come on top): hot and cold sources,
    messages fed to completion in any order, duplicates, inconsistent totals, records that are no fragments, forged headers, clock
    steps in both directions, gc calls.  Codes, tag lists, msg_len, pending and released
    must be those of the restatement."""
    rng = random.Random(seed)
    p = _Pair()
    hot = [b"10.0.0.%d:%d" % (i, 4000 + i) for i in range(6)]
    cold = [b"[2001:db8::%x]:443" % i for i in range(900)]
    plans, now, peak, evicted, expired = [], 1000, 1000, 0, 0
    step = -1
    while p.tag < 20000:   # p.tag counts the feeds
        step += 1
        if step % 200 == 0:
            evicted += len(p.check())   # between two gc calls: dropped by evictions
        x = rng.random()
        if step < 5000 or x < 0.30:   # a new message (the first 5000: the table fills and evicts)
            src = rng.choice(hot) if rng.random() < 0.15 else rng.choice(cold)
            total = rng.randint(2, 8)
            order = list(range(total))
            rng.shuffle(order)
            plans.append([src, rng.randrange(256) if src in cold else rng.randrange(12), total, order])
            if len(plans) > 40:
                plans.pop(rng.randrange(len(plans)))   # some are never finished
            if step < 5000:   # its first chunk at once: 5000 new keys, more than the table holds
                p.feed(src, gecko.FRAGMENT, plans[-1][1], order.pop(), total, 100, now)
                if step % 10:
                    plans.pop()
                continue
        if plans and x < 0.80:
            pl = rng.choice(plans)
            src, mid, total, order = pl
            y = rng.random()
            if y < 0.08:     # a duplicate or a chunk of a message that is done
                p.feed(src, gecko.FRAGMENT, mid, rng.randrange(total), total, rng.randrange(1500), now)
            elif y < 0.12:   # another total for the same key
                t2 = rng.randint(2, 8)
                p.feed(src, gecko.FRAGMENT, mid, rng.randrange(t2), t2, 7, now)
            else:
                st, tags, _ = p.feed(src, gecko.FRAGMENT, mid, order.pop(), total, rng.choice((0, 1, 600, 1187)), now)
                if not order:
                    plans.remove(pl)
        elif x < 0.86:
            p.feed(rng.choice(cold), gecko.PASS, payload_len=rng.randrange(1, 1400), now=now)
        elif x < 0.92:   # not a fragment, or one decodeFrame could not have produced
            st = rng.choice((gecko.EMPTY, gecko.ERR_TRUNCATED, gecko.ERR_INVALID, gecko.FRAGMENT, gecko.FRAGMENT))
            total = rng.choice((0, 1, 9, 15, 4))
            p.feed(rng.choice(hot), st, 3, rng.choice((total, 15)), total, 5, now)
        elif x < 0.97:
            now = max(0, now + rng.choice((0, 1, 100, 3999, 4000, 8000, 8001, -50)))
            peak = max(peak, now)
        else:
            p.gc(now)
            expired += len(p.check())
    p.gc(peak + R.TTL_MS + 1)   # past every deadline: the clock also stepped back
    p.check()
    assert p.c.pending() == 0
    assert p.tag >= 20000 and sum(p.codes.values()) == p.tag
    assert evicted > 100 and expired > 100
    assert p.codes[R.COMPLETE] > 300 and p.codes[R.DROPPED] > 1000 and p.codes[R.PASS] > 300 and p.codes[R.PENDING] > 5000


def _frag(r, src, mid, idx, total, tag, now=0, ln=10):
    return r.feed(src, _rec(gecko.FRAGMENT, mid, idx, total, 3, ln), tag, now)


def test_reassembles_out_of_order():
    """TestGeckoReassemblesOutOfOrder: tags come back in chunk order, msg_len is the sum."""
    r = gecko.Reassembler()
    for idx, tag in ((2, 30), (0, 10), (3, 40)):
        assert _frag(r, b"a:1", 7, idx, 4, tag, ln=idx + 1) == (R.PENDING, [], 0)
    assert r.pending() == 1
    assert _frag(r, b"a:1", 7, 1, 4, 20, ln=2) == (R.COMPLETE, [10, 20, 30, 40], 1 + 2 + 3 + 4)
    assert r.pending() == 0 and r.released() == []


def test_expiry_is_strict_and_never_refreshed():
    """TestGeckoExpiresIncompleteFragment: gone after now + TTL, not at it; a later chunk
    does not move the deadline."""
    r = gecko.Reassembler()
    _frag(r, b"a:1", 1, 0, 3, 100, now=5000)
    _frag(r, b"a:1", 1, 1, 3, 101, now=9000)
    r.gc(5000 + gecko.REASSEMBLY_TTL_MS)
    assert r.pending() == 1 and r.released() == []
    r.gc(5000 + gecko.REASSEMBLY_TTL_MS + 1)
    assert r.pending() == 0 and r.released() == [100, 101] and r.released() == []
    assert _frag(r, b"a:1", 1, 2, 3, 102, now=14000) == (R.PENDING, [], 0)   # a new entry: the others are gone


def test_per_source_cap():
    """TestGeckoEnforcesPerSourceCap: the ninth message of a source is dropped, and
    accepted again once one of the eight completes; other sources are not affected."""
    r = gecko.Reassembler()
    for mid in range(8):
        assert _frag(r, b"a:1", mid, 0, 2, mid)[0] == R.PENDING
    assert _frag(r, b"a:1", 8, 0, 2, 99)[0] == R.DROPPED
    assert _frag(r, b"a:2", 8, 0, 2, 98)[0] == R.PENDING
    assert _frag(r, b"a:1", 3, 0, 2, 97)[0] == R.DROPPED      # a duplicate of a pending one: still dropped
    assert _frag(r, b"a:1", 3, 1, 2, 50) == (R.COMPLETE, [3, 50], 20)
    assert _frag(r, b"a:1", 8, 0, 2, 96)[0] == R.PENDING
    assert r.pending() == 9


def test_global_cap_evicts_the_oldest():
    """TestGeckoEvictsOldestOnGlobalCap, through feed: distinct sources, deadlines one
    millisecond apart, created in descending order of deadline."""
    r = gecko.Reassembler()
    n = gecko.MAX_REASSEMBLY
    for i in range(n):
        assert _frag(r, b"src-%d" % i, 1, 0, 4, i, now=n - i)[0] == R.PENDING
    assert r.pending() == n and r.released() == []
    assert _frag(r, b"new", 1, 0, 4, 5000, now=10 * n)[0] == R.PENDING
    assert r.pending() == n and r.released() == [n - 1]       # the smallest deadline: the last one created
    assert _frag(r, b"src-%d" % (n - 1), 1, 1, 4, 5001, now=10 * n)[0] == R.PENDING   # its source starts anew
    assert r.released() == [n - 2]


def test_global_cap_tie_goes_to_the_first_created():
    r = gecko.Reassembler()
    n = gecko.MAX_REASSEMBLY
    for i in range(n):
        _frag(r, b"src-%d" % i, 1, 0, 4, i, now=77)
        if i < 3:
            _frag(r, b"src-%d" % i, 1, 2, 4, 10000 + i, now=77)
    for k in range(3):
        _frag(r, b"more-%d" % k, 1, 0, 4, 20000 + k, now=76 if k == 2 else 77)   # the last: an earlier deadline
    assert r.released() == [0, 10000, 1, 10001, 2, 10002]      # equal deadlines: in creation order; chunk order within
    _frag(r, b"again", 1, 0, 4, 30000, now=77)
    assert r.released() == [20002]                             # the earliest deadline beats creation order
    assert r.pending() == n


def test_bounded_under_garbage_flood():
    """TestGeckoBoundedUnderGarbageFlood: 50 000 random datagrams (seed 42) from 4096
    addresses; the table stays within both caps."""
    rng = random.Random(42)
    r, ref = gecko.Reassembler(), R.Conn()
    for i in range(50000):
        junk = rng.randbytes(16 + rng.randrange(200))
        src = b"10.0.0.%d:%d" % (i % 256, 1024 + i % 4096)
        kind, h, payload = gref.parse(junk)
        if kind == gref.FRAGMENT:
            rec = _rec(gecko.FRAGMENT, h.msg_id, h.chunk_idx, h.total_chunks, h.pad_len, len(payload))
            want = ref.feed(src, kind, h.msg_id, h.chunk_idx, h.total_chunks, len(payload), i, i // 10)
        else:
            rec = _rec(gc.STATUS[kind], payload_len=len(junk) if kind == gref.PASS else 0)
            want = ref.feed(src, kind, 0, 0, 0, len(junk), i, i // 10)
        assert r.feed(src, rec, i, i // 10) == want
    assert 0 < r.pending() == len(ref.reassembly) <= gecko.MAX_REASSEMBLY
    assert max(ref.per_source.values()) <= gecko.MAX_PER_SOURCE
    assert r.released() == ref.take_released()


def test_chunk_after_completion_starts_a_new_entry():
    r = gecko.Reassembler()
    _frag(r, b"a:1", 5, 0, 2, 1)
    assert _frag(r, b"a:1", 5, 1, 2, 2)[0] == R.COMPLETE
    assert _frag(r, b"a:1", 5, 1, 2, 3) == (R.PENDING, [], 0) and r.pending() == 1
    assert _frag(r, b"a:1", 5, 0, 2, 4, ln=1) == (R.COMPLETE, [4, 3], 11)


def test_feed_answers_for_records_that_are_no_fragments():
    r = gecko.Reassembler()
    assert r.feed(b"", _rec(gecko.PASS, payload_len=1192), 9, 0) == (R.PASS, [9], 1192)
    for st in (gecko.EMPTY, gecko.ERR_TRUNCATED, gecko.ERR_INVALID):
        assert r.feed(b"x", _rec(st), 9, 0) == (R.DROPPED, [], 0)
    for idx, total in ((0, 0), (0, 1), (0, 9), (2, 2), (15, 8)):
        assert _frag(r, b"x", 1, idx, total, 9) == (R.DROPPED, [], 0)
    assert r.pending() == 0
    assert _frag(r, b"", 1, 0, 2, 9)[0] == R.PENDING and _frag(r, b"\0", 1, 0, 2, 9)[0] == R.PENDING   # sources are bytes
    assert r.pending() == 2


def test_null_arguments_and_empty_batches():
    lib = gecko._glib()
    N = None
    assert lib.hyobfs_abi_version() == 4
    assert lib.hyobfs_gecko_peek_batch(N, N, N, N, 0, N, N, N) == 0
    assert lib.hyobfs_gecko_open_batch(N, N, N, N, N, 0, N, N, 0, N, N, N, N, N, N) == 0
    assert lib.hyobfs_gecko_open_batch(N, N, N, N, N, 7, N, N, 0, N, N, N, N, N, N) == 0
    assert lib.hyobfs_gecko_peek_batch(N, N, N, N, 1, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_gecko_open_batch(N, N, N, N, N, 0, N, N, 1, N, N, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    r = gecko.Reassembler()
    n = gecko.ctypes.c_uint32()
    tags = (gecko.ctypes.c_uint64 * 8)()
    rec = _rec(gecko.PASS, payload_len=3)
    args = [r._h, b"a", 1, rec, 1, 0, gecko.ctypes.addressof(tags), gecko.ctypes.byref(n), gecko.ctypes.byref(n)]
    for k in (0, 1, 3, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert lib.hyobfs_gecko_reassembler_feed(*bad) == _lib.HYOBFS_ERR_INVALID, k
    assert lib.hyobfs_gecko_reassembler_feed(r._h, None, 0, rec, 1, 0, *args[6:]) == gecko.RX_PASS
    lib.hyobfs_gecko_reassembler_free(N)
    lib.hyobfs_gecko_reassembler_gc(N, 0)
    assert lib.hyobfs_gecko_reassembler_pending(N) == 0 and lib.hyobfs_gecko_reassembler_released(N, N, 0) == 0


# ------------------------------------------------------------------ the header
def test_header_is_c11_and_the_new_codes_are_free(tmp_path):
    """include/hyobfs_gecko.h compiles as C11; the new constants have the stated values,
    which no other status code of include/*.h has."""
    import re
    names = ["HYOBFS_GECKO_ERR_CAP", "HYOBFS_GECKO_ERR_PLAN", "HYOBFS_GECKO_RX_PENDING", "HYOBFS_GECKO_RX_PASS",
             "HYOBFS_GECKO_RX_COMPLETE", "HYOBFS_GECKO_RX_DROPPED", "HYOBFS_GECKO_REASSEMBLY_TTL_MS",
             "HYOBFS_GECKO_MAX_REASSEMBLY", "HYOBFS_GECKO_MAX_PER_SOURCE", "HYOBFS_ABI_VERSION"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hyobfs_gecko.h"\nint main(void){\n' +
                   "\n".join('printf("%%d\\n", (int)%s);' % c for c in names) +
                   '\nprintf("%zu\\n", sizeof(hyobfs_gecko_parsed));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [-23, -24, 0, 1, 2, 3, 8000, 4096, 8, 4, 16]
    assert (gecko.ERR_CAP, gecko.ERR_PLAN, gecko.RX_PENDING, gecko.RX_PASS, gecko.RX_COMPLETE, gecko.RX_DROPPED,
            gecko.REASSEMBLY_TTL_MS, gecko.MAX_REASSEMBLY, gecko.MAX_PER_SOURCE) == tuple(vals[:9])
    assert (gc.ERR_CAP, gc.ERR_PLAN, R.PENDING, R.PASS, R.COMPLETE, R.DROPPED, R.TTL_MS) == tuple(vals[:7])
    codes = {}
    for fn in sorted(os.listdir(os.path.join(ROOT, "include"))):
        for name, v in re.findall(r"#define\s+(HYOBFS_\w+)\s+\((-\d+)\)", open(os.path.join(ROOT, "include", fn)).read()):
            codes.setdefault(int(v), []).append(name)
    assert codes[-23] == ["HYOBFS_GECKO_ERR_CAP"] and codes[-24] == ["HYOBFS_GECKO_ERR_PLAN"]
    assert len(codes) > 40 and all(len(v) == 1 for v in codes.values()), [v for v in codes.values() if len(v) > 1]


def test_package_exports():
    import hysteria_amd
    assert "GeckoReceiver" in hysteria_amd.__all__ and hysteria_amd.GeckoReceiver is gecko.GeckoReceiver
    for name in ("peek_batch", "open_batch", "Reassembler", "GeckoReceiver"):
        assert hasattr(gecko, name)
    assert gc.PARSED_DTYPE == gecko.PARSED_DTYPE


# ------------------------------------------------------------------ the builders' own conditions
def test_lattices_meet_their_conditions():
    cases = gc.peek_cases()
    whole = cases[0]
    assert {int(o) % 16 for o in whole["off"]} == set(range(16))
    assert {0, 1, 7, 8, 9, 10, 12, 13, 14} <= set(whole["len"].tolist())
    assert int((whole["off"] + whole["len"]).max()) == whole["buf_len"]    # no slack
    recs, keys = gc.expected_peek(whole)
    assert set(recs["status"].tolist()) == {gc.PASS, gc.FRAGMENT, gc.EMPTY, gc.TRUNCATED, gc.INVALID}
    frag = recs[recs["status"] == gc.FRAGMENT]
    assert {0, 1, 65535} <= set(frag["pad_len"].tolist()) and 0 in frag["payload_len"] and 3 in frag["payload_len"]
    assert {0x02, 0x12, 0x08, 0x78} <= set(frag["idx_total"].tolist())
    assert (keys[whole["len"] <= 8] == gc.GUARD).all() and len(whole["wires"]) >= 257
    assert [len(c["wires"]) for c in cases[2:7]] == list(gc.PEEK_NS)
    assert [len(c["psk"]) for c in cases[7:]] == list(gc.PSK_LENS)
    for c in cases[7:]:   # every kind is there under every PSK
        assert set(gc.expected_peek(c)[0]["status"].tolist()) == {gc.PASS, gc.FRAGMENT, gc.EMPTY, gc.TRUNCATED, gc.INVALID}
    ocs = gc.open_cases()
    assert [len(c["lists"]) for c in ocs[:5]] == list(gc.OPEN_MS)
    pool = ocs[4]
    st, ln, out = gc.expected_open(pool)
    assert set(st.tolist()) == {gc.OK, gc.ERR_CAP}
    ok = [l for l, s in zip(pool["lists"], st) if s == gc.OK]
    assert {len(l) for l in ok} >= set(range(1, 9)) and any(len(set(l)) < len(l) for l in ok)
    assert any(l == sorted(l, reverse=True) and len(l) > 2 for l in ok) and any(max(l) - min(l) > len(l) for l in ok)
    used = pool["recs"][sorted({i for l in ok for i in l})]
    assert set(used["payload_len"].tolist()) >= set(gc.OPEN_LENS)
    assert {int(x) % 32 for x in used["payload_off"]} == set(range(32))
    for c in ocs:   # the expectation opens every message to the bytes that were put in
        st, ln, out = gc.expected_open(c)
        for j, (s, w) in enumerate(zip(st, c["want"])):
            if s == gc.OK:
                assert out[int(c["out_off"][j]):int(c["out_off"][j]) + len(w)].tobytes() == w and ln[j] == len(w)
        assert (c["gaps"] >= 1).all()
    res = ocs[5]
    seen = set()
    for j, l in enumerate(res["lists"]):
        for i in l:
            po = int(res["recs"][i]["payload_off"])
            seen.add(((int(res["off"][i]) + 8 + po) % 16, int(res["out_off"][j]) % 16, po % 32))
    assert len(seen) == 16 * 16 * 32
    plan = ocs[6]
    assert list(gc.expected_open(plan)[0]) == plan["exp"] and plan["exp"].count(gc.ERR_PLAN) == len(plan["labels"]) == 17


# ------------------------------------------------------------------ the kernels on the CPU
@pytest.fixture(scope="module")
def rx_main():
    """tests/emu/build/gecko_rx_main, rebuilt when the driver, the header or the emulated
    library is newer."""
    if not os.path.exists(CLANG):
        pytest.fail("no host clang: the only sanitizer coverage of the peek and open kernels cannot run")
    lib = emu_build.ensure_emu_lib()
    src = os.path.join(EMU, "gecko_rx_main.cpp")
    deps = [src, lib] + [os.path.join(ROOT, "include", h) for h in ("hyobfs.h", "hyobfs_gecko.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "gecko_rx_main")
    with open(os.path.join(EMU, "build", ".gecko_rx_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            src, "-L" + EMU, "-lhyobfs_emu", "-Wl,-rpath," + EMU, "-o", tmp], check=True,
                           capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, blob: bytes) -> bytes:
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(blob)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.splitlines()[-1:] == ["done"], r.stderr[-4000:]
    return dst.read_bytes()


class _Reader:
    def __init__(self, b):
        self.b, self.at = b, 0

    def arr(self, dtype, n):
        a = np.frombuffer(self.b, dtype, n, self.at)
        self.at += a.nbytes
        return a

    def done(self):
        return self.at == len(self.b)


def test_emulated_peek_lattice(rx_main, tmp_path):
    """Every case of the peek lattice: records against gecko_ref.parse of salamander_ref's
    deobfuscation, keys against hashlib's BLAKE2b, the keys of datagrams without plaintext
    untouched; the wire buffer without slack and, where slotted, poisoned between slots."""
    cases = gc.peek_cases()
    res = _Reader(_run(rx_main, tmp_path, b"".join(gc.blob_peek(c) for c in cases)))
    for c in cases:
        n = len(c["wires"])
        assert int(res.arr(np.int32, 1)[0]) == 0, c["name"]
        gc.check_peek(c, res.arr(np.uint8, 16 * n), res.arr(np.uint8, 32 * n))
    assert res.done()


@pytest.mark.parametrize("which", ["pool", "residues", "plan errors"])
def test_emulated_open_lattice(rx_main, tmp_path, which):
    """Statuses, out_len and the whole output buffer, guard bytes included, of every case."""
    cases = [c for c in gc.open_cases() if c["name"].startswith(which)]
    assert cases
    res = _Reader(_run(rx_main, tmp_path, b"".join(gc.blob_open(c) for c in cases)))
    for c in cases:
        m = len(c["lists"])
        assert int(res.arr(np.int32, 1)[0]) == 0, c["name"]
        status, out_len = res.arr(np.int32, m), res.arr(np.uint32, m)
        total = int(res.arr(np.uint64, 1)[0])
        assert total == c["out_total"]
        gc.check_open(c, status, out_len, res.arr(np.uint8, total))
    assert res.done()
