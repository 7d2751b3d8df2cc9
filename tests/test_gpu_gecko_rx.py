"""Gecko's receive path on the GPU (include/hyobfs_gecko.h): the peek and open
lattices of tests/gecko_rx_cases.py through the ABI, the round trip encode -> peek ->
Reassembler -> open, parity of peek with today's deobfuscate + parse, and GeckoReceiver
against the host GeckoPacketConn on one datagram stream."""
import random

import numpy as np
import pytest

from oracle import gecko_ref as gref
from oracle import salamander_ref as sref

import gecko_rx_cases as gc
from hysteria_amd.gecko import GeckoReceiver, Reassembler, open_batch, peek_batch  # noqa: F401  (the feature under test)

pytestmark = pytest.mark.gpu
PSK = gc.PSK
KEY, NONCE = bytes(range(7, 39)), bytes(range(100, 112))


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.array(a, copy=True).view(np.uint8)).to(gpu)   # writable copy, as bytes: only the pointer counts


def _guarded(nbytes, gpu):
    import torch
    return torch.full((max(nbytes, 1),), gc.GUARD, dtype=torch.uint8, device=gpu)


def _peek(o, gpu, buf, off, lens):
    from hysteria_amd import gecko
    n = len(lens)
    parsed, keys = _guarded(16 * n, gpu), _guarded(32 * n, gpu)
    gecko.peek_batch(o, _dev(buf, gpu), _dev(off, gpu), _dev(lens, gpu), n, parsed, keys)
    return parsed, keys


# ------------------------------------------------------------------ the lattices through the ABI
def test_peek_lattice(gpu):
    """All 16 bytes of every record and every key of every case (lengths around the salt
    and the header, every header field at its edges, every offset residue, n around the
    workgroup size, every salt word and the two-block key); the key ranges of datagrams
    without plaintext untouched."""
    import hysteria_amd
    for case in gc.peek_cases():
        with hysteria_amd.SalamanderObfuscator(case["psk"], 0) as o:
            parsed, keys = _peek(o, gpu, gc.wire_buffer(case), case["off"], case["len"])
            n = len(case["wires"])
            gc.check_peek(case, parsed.cpu().numpy()[:16 * n], keys.cpu().numpy()[:32 * n])


def _open(gpu, case):
    from hysteria_amd import gecko
    m = len(case["lists"])
    out, out_len, status = _guarded(case["out_total"], gpu), _guarded(4 * m, gpu), _guarded(4 * m, gpu)
    gecko.open_batch(_dev(gc.wire_buffer(case), gpu), _dev(case["off"], gpu), _dev(case["len"], gpu), _dev(case["recs"], gpu),
                     _dev(case["keys"], gpu), len(case["wires"]), _dev(case["idx"], gpu), _dev(case["first"], gpu), m, out,
                     _dev(case["out_off"], gpu), _dev(case["caps"], gpu), out_len, status)
    return (status.cpu().numpy()[:4 * m].view(np.int32), out_len.cpu().numpy()[:4 * m].view(np.uint32),
            out.cpu().numpy()[:case["out_total"]])


@pytest.mark.parametrize("which", ["pool", "residues", "plan errors"])
def test_open_lattice(gpu, which):
    """Statuses, out_len and the whole output, guard bytes on both sides of every message
    included: totals 2..8 and single PASS lists, the payload lengths around the window
    size, reversed and distant slots, a slot named twice, capacities exact and one short,
    the three residues crossed, every ERR_PLAN cause."""
    cases = [c for c in gc.open_cases() if c["name"].startswith(which)]
    assert cases
    for case in cases:
        gc.check_open(case, *_open(gpu, case))


# ------------------------------------------------------------------ round trip
def _encoded(gpu, o, n_msgs, seed):
    """(messages, wire datagrams, the message of each datagram) of n_msgs long-header
    messages through plan_fragments + encode_batch; lengths 1, 5, 27 and 2000 among them."""
    import torch
    from hysteria_amd import gecko
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 1400, n_msgs)
    lens[:4] = [1, 5, 27, 2000]
    msg = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    fr, off, total = gecko.plan_fragments(lens, 512, 1200, first_msg_id=0,
                                          rand32=lambda k: rng.integers(0, 2**32, k, dtype=np.uint64))
    nf = len(fr)
    wire = torch.empty(total + 16, dtype=torch.uint8, device=gpu)
    gecko.encode_batch(o, msg=_dev(msg, gpu), frames=_dev(fr, gpu), salts=_dev(sref.splitmix64_array(seed, 0, nf), gpu),
                       pad_key=KEY, pad_nonce=NONCE, out=wire, out_off=_dev(off, gpu), n=nf)
    h = wire.cpu().numpy()
    wl = 13 + fr["chunk_len"].astype(np.int64) + fr["pad_len"]
    base = np.concatenate([[0], np.cumsum(lens)])
    msgs = [msg[base[m]:base[m + 1]].tobytes() for m in range(n_msgs)]
    owner, m = [], -1
    for f in fr:
        m += (int(f["idx_total"]) >> 4) == 0
        owner.append(m)
    return msgs, [h[int(off[i]):int(off[i]) + int(wl[i])].tobytes() for i in range(nf)], owner


def _short_headers(gpu, o, n, seed):
    """n short-header packets (top bit clear) obfuscated by the batch call: (plain, wire)."""
    import torch
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 1300, n).astype(np.uint32)
    plain = [bytes([int(rng.integers(0, 128))]) + rng.integers(0, 256, int(ln) - 1, dtype=np.uint8).tobytes() for ln in lens]
    buf = np.frombuffer(b"".join(plain), np.uint8)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = torch.empty(int(lens.sum()) + 8 * n, dtype=torch.uint8, device=gpu)
    ooff = torch.empty(n, dtype=torch.int64, device=gpu)
    olen = torch.empty(n, dtype=torch.int32, device=gpu)
    import hysteria_amd
    ws = torch.empty(hysteria_amd.workspace_size(n), dtype=torch.uint8, device=gpu)
    o.obfuscate_batch(_dev(buf, gpu), n, in_off=torch.from_numpy(off).to(gpu), in_len=torch.from_numpy(lens.view(np.int32)).to(gpu),
                      salts=torch.from_numpy(sref.splitmix64_array(seed, 0, n).view(np.int64)).to(gpu), out=out,
                      out_cap=out.numel(), out_off=ooff, out_len=olen, workspace=ws, workspace_bytes=ws.numel())
    h, ho, hl = out.cpu().numpy(), ooff.cpu().numpy(), olen.cpu().numpy()
    return plain, [h[int(ho[i]):int(ho[i]) + int(hl[i])].tobytes() for i in range(n)]


def test_round_trip_encode_peek_reassemble_open(gpu):
    """300 fragmented messages and 60 short-header datagrams, shuffled: peek, the C
    reassembler over the records, one open: every message byte-exact, in completion order."""
    import hysteria_amd
    from hysteria_amd import gecko
    with hysteria_amd.SalamanderObfuscator(PSK, 0) as o:
        msgs, frames, owner = _encoded(gpu, o, 300, 21)
        shorts, swire = _short_headers(gpu, o, 60, 22)
        items = [(w, ("frag", owner[i])) for i, w in enumerate(frames)] + [(w, ("short", i)) for i, w in enumerate(swire)]
        random.Random(3).shuffle(items)
        wires = [w for w, _ in items]
        lens = np.array([len(w) for w in wires], np.uint32)
        off, total = gc.packed(lens.tolist())
        buf = np.frombuffer(b"".join(wires), np.uint8)
        d_buf, d_off, d_len = _dev(buf, gpu), _dev(off, gpu), _dev(lens, gpu)
        n = len(wires)
        parsed, keys = _guarded(16 * n, gpu), _guarded(32 * n, gpu)
        gecko.peek_batch(o, d_buf, d_off, d_len, n, parsed, keys)
        recs = parsed.cpu().numpy().view(gecko.PARSED_DTYPE)
        r = gecko.Reassembler()
        lists, caps, want = [], [], []
        for i, (_, (kind, k)) in enumerate(items):   # one source per message: 300 shuffled messages of one source
            st, tags, ln = r.feed(b"src-%d" % k if kind == "frag" else b"short", recs[i], i, 0)   # would hit its cap of 8
            if st in (gecko.RX_PASS, gecko.RX_COMPLETE):
                lists.append(tags)
                caps.append(ln)
                want.append(msgs[k] if kind == "frag" else shorts[k])
            else:
                assert st == gecko.RX_PENDING
        assert r.pending() == 0 and len(lists) == 360
        m = len(lists)
        first = np.zeros(m + 1, np.uint64)
        np.cumsum([len(l) for l in lists], out=first[1:])
        out_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
        out, out_len, status = _guarded(sum(caps) + 32, gpu), _guarded(4 * m, gpu), _guarded(4 * m, gpu)
        gecko.open_batch(d_buf, d_off, d_len, parsed, keys, n, _dev(np.array([t for l in lists for t in l], np.uint32), gpu),
                         _dev(first, gpu), m, out, _dev(out_off, gpu), _dev(np.array(caps, np.uint32), gpu), out_len, status)
        h = out.cpu().numpy()
        assert not status.cpu().numpy().view(np.int32).any()
        assert out_len.cpu().numpy().view(np.uint32).tolist() == [len(w) for w in want]
        assert h[:sum(caps)].tobytes() == b"".join(want) and (h[sum(caps):] == gc.GUARD).all()
        assert {1, 5, 27, 2000} <= {len(w) for w in want}


def test_peek_equals_deobfuscate_then_parse(gpu):
    """For the same wire -- the whole peek lattice and an encoded batch -- the records of
    peek_batch are those of deobfuscate_batch followed by parse_batch, all 16 bytes."""
    import torch
    import hysteria_amd
    from hysteria_amd import gecko
    with hysteria_amd.SalamanderObfuscator(PSK, 0) as o:
        _, frames, _ = _encoded(gpu, o, 40, 31)
        case = gc.peek_cases()[0]
        wires = case["wires"] + frames
        lens = np.array([len(w) for w in wires], np.uint32)
        off, total = gc.packed(lens.tolist())
        n = len(wires)
        d_buf, d_off, d_len = _dev(np.frombuffer(b"".join(wires), np.uint8), gpu), _dev(off, gpu), _dev(lens, gpu)
        parsed, keys = _guarded(16 * n, gpu), _guarded(32 * n, gpu)
        gecko.peek_batch(o, d_buf, d_off, d_len, n, parsed, keys)
        plain = torch.empty(total + 16, dtype=torch.uint8, device=gpu)
        poff = torch.empty(n, dtype=torch.int64, device=gpu)
        plen = torch.empty(n, dtype=torch.int32, device=gpu)
        ws = torch.empty(hysteria_amd.workspace_size(n), dtype=torch.uint8, device=gpu)
        o.deobfuscate_batch(d_buf, n, in_off=d_off.view(torch.int64), in_len=d_len.view(torch.int32), out=plain, out_cap=total,
                            out_off=poff, out_len=plen, workspace=ws, workspace_bytes=ws.numel())
        today = _guarded(16 * n, gpu)
        gecko.parse_batch(plain, poff, plen, n, today)
        a, b = parsed.cpu().numpy().view(gecko.PARSED_DTYPE), today.cpu().numpy().view(gecko.PARSED_DTYPE)
    bad = [i for i in range(n) if a[i].tobytes() != b[i].tobytes()]
    assert not bad, [(i, a[i], b[i]) for i in bad[:4]]
    assert set(a["status"].tolist()) == {gecko.PASS, gecko.FRAGMENT, gecko.EMPTY, gecko.ERR_TRUNCATED, gecko.ERR_INVALID}


# ------------------------------------------------------------------ the pipeline against the host conn
def _stream(seed=9):
    """About 2000 wire datagrams from 5 sources: fragmented messages whose chunks mix with
    those of their neighbours, duplicates, short-header packets, garbage, datagrams without
    plaintext, and one message that lacks a chunk."""
    rng = random.Random(seed)
    srcs = [("10.1.0.%d" % i, 5000 + i) for i in range(5)]
    next_id = [0] * 5
    out, window, k = [], [], 0

    def wire(plain):
        nonlocal k
        k += 1
        return sref.obfuscate(PSK, plain, sref.splitmix64_at(seed, k).to_bytes(8, "little"))

    for m in range(330):
        s = rng.randrange(5)
        data = bytes([0xC0 | rng.randrange(64)]) + rng.randbytes(rng.choice((0, 4, 26, 600, 1199, 1999)))
        total = rng.randint(2, 8)
        mid = next_id[s] & 0xFF
        next_id[s] += 1
        for i, (a, b) in enumerate(gref.split_chunks(len(data), total)):
            if m == 200 and i == 1:
                continue   # the incomplete one
            pad = gref.pad_len(512, 1200, b - a, rng.getrandbits(32))
            window.append((wire(gref.encode_frame(gref.Header(pad, mid, i, total), data[a:b], rng.randbytes(pad))), srcs[s]))
        if m % 3 == 2 or m == 329:   # the chunks of three messages, mixed
            rng.shuffle(window)
            for w in window:
                out.append(w)
                x = rng.random()
                if x < 0.06:
                    out.append(rng.choice(window))                                 # a duplicate
                elif x < 0.10:
                    out.append((wire(bytes([rng.randrange(128)]) + rng.randbytes(rng.randrange(1200))), rng.choice(srcs)))
                elif x < 0.14:
                    out.append((rng.randbytes(9 + rng.randrange(60)), rng.choice(srcs)))   # garbage
                elif x < 0.15:
                    out.append((rng.randbytes(rng.randrange(9)), rng.choice(srcs)))        # no plaintext
            window = []
    return out


class _Inner:
    """What the Salamander conn under a GeckoPacketConn delivers for a wire stream."""

    def __init__(self, stream):
        self.it = iter(stream)

    def read_from(self, bufsize):
        w, addr = next(self.it)   # StopIteration ends the run
        return sref.deobfuscate(PSK, w), addr

    def close(self):
        pass


def test_receiver_against_packet_conn(gpu):
    """The same stream through GeckoPacketConn (host, deobfuscated datagrams) and through
    GeckoReceiver in pushes of 1, 7 and 64 datagrams, so that messages straddle pushes:
    equal (payload, addr) sequences; afterwards every slot is free or pinned."""
    import hysteria_amd
    from hysteria_amd import gecko
    stream = _stream()
    assert 1800 < len(stream) < 2400
    conn, want = gecko.GeckoPacketConn(_Inner(stream)), []
    try:
        while True:
            want.append(conn.read_from())
    except (StopIteration, RuntimeError):
        pass
    left = len(conn.reassembly)
    conn.close()
    assert len(want) > 350 and left >= 1
    with hysteria_amd.SalamanderObfuscator(PSK, 0) as o:
        rx = gecko.GeckoReceiver(o, max_batch=64)
        got, at, sizes = [], 0, (1, 7, 64)
        while at < len(stream):
            k = sizes[(at // 3) % 3]
            part = stream[at:at + k]
            got += rx.push([w for w, _ in part], [a for _, a in part], now_ms=1000 + at)
            at += k
        assert got == want
        assert rx.pending() == left and rx.pinned_slots >= left
        assert rx.free_slots + rx.pinned_slots == rx.slots
        rx.gc(1000 + len(stream) + gecko.REASSEMBLY_TTL_MS + 1)
        assert rx.pending() == 0 and rx.pinned_slots == 0 and rx.free_slots == rx.slots
        rx.close()
